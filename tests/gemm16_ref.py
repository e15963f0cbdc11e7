"""float64 definitions of the four launches of csrc/vc_gemm16.hip (include/vc_hip.h "f16x3"), numpy only.

gemm16(d) restates vc_gemm16 from the float16 planes themselves:

    acc = conv(x_hi, w_hi) + conv(x_hi, w_lo) + conv(x_lo, w_hi)          (there is no lo * lo term)
    out = act(acc * row_scale * col_scale + col_shift) (+ the old contents)

SAME padding per window of T rows.  split16 / transpose_split16 / weights16 are the bit model of the operand kernels:
one power of two per window / channel / group from the largest magnitude after affine and relu and BEFORE the pool,
hi = float16(x s), lo = float16(x s - hi), round to nearest even, subnormals kept.

A descriptor is a dict (tests/gemm16_cases.py builds them):
  M, T, C, ldx, X16 [M, ldx] float16 ([hi (C) | lo (C) | padding]), row_scale / col_scale / col_shift (arrays or None),
  ragged, pairs = [dict(Bt0, Bt1, taps0, extra, pad_l, c_off0, c_off1, row0, nrows0, nrows1, s_off0, s_off1)],
  ldc, nbuf (elements of the output buffer), accumulate, act, atomic_splits.
The output buffer is FLAT: element (row r of a pair, column n of filter f) is r * ldc + c_off_f + n in both forms (the
atomic form's c_off are element offsets), so one function serves both and columns nobody stores are part of every
comparison.

The launcher's host rules (choose_ksplit, the forced option, split_cs, the 16-pair map, tl / seg of vc_split16) are
restated at the end, each with the line of vc_gemm16.hip it restates."""
import numpy as np

ACT_NONE, ACT_RELU = 0, 1
BM, MAX_SPLIT = 256, 8
F64 = np.float64


# --------------------------------------------------------------------------------------------------------------------
# vc_gemm16

def pair_rows(d, p):
    """(nrows0, nrows1) as the launcher resolves them: 0 = M - row0, nrows1 = -1 = nothing stored."""
    n0 = p['nrows0'] if p['nrows0'] else d['M'] - p['row0']
    n1 = 0 if p['nrows1'] < 0 else (p['nrows1'] if p['nrows1'] else d['M'] - p['row0'])
    return n0, n1


def _filters(d, p):
    """[(Bt, taps, nrows, c_off, s_off, is_first)] of a pair."""
    n0, n1 = pair_rows(d, p)
    atomic = d.get('atomic_splits', 0) >= 1
    s0, s1 = (p['s_off0'], p['s_off1']) if atomic else (p['c_off0'], p['c_off1'])
    return [(p['Bt0'], p['taps0'], n0, p['c_off0'], s0, True), (p['Bt1'], p['taps0'] + p['extra'], n1, p['c_off1'], s1, False)]


def stored_mask(d):
    """bool [nbuf]: the elements the launch stores (or adds to)."""
    m = np.zeros(d['nbuf'], bool)
    for p in d['pairs']:
        for Bt, taps, nrows, c_off, s_off, first in _filters(d, p):
            if nrows > 0:
                idx = (np.arange(nrows)[:, None] * d['ldc'] + c_off + np.arange(128)[None, :]).ravel()
                assert idx.min() >= 0 and idx.max() < d['nbuf'], 'case stores outside its buffer'
                m[idx] = True
    return m


def _shifted(plane, rows, sh, T):
    """rows `rows` of `plane` read sh frames later, 0 where that leaves the row's window (selected, never multiplied)."""
    t = rows % T
    ok = (t + sh >= 0) & (t + sh < T)
    src = np.clip(rows + sh, 0, plane.shape[0] - 1)
    return np.where(ok[:, None], plane[src], 0.0)


def _acc_uniform(d, p, Bt, taps, nrows, first, mix, absolute):
    C, T = d['C'], d['T']
    X = d['X16'].astype(F64)
    xh, xl = X[:, :C], X[:, C:2 * C]
    if mix == 'swap_x_planes':
        xh, xl = xl, xh
    W = np.asarray(Bt).astype(F64)[:, :taps * 2 * C].reshape(128, taps, 2, C)
    if absolute:
        xh, xl, W = np.abs(xh), np.abs(xl), np.abs(W)
    rows = p['row0'] + np.arange(nrows)
    pad = p['pad_l'] + (1 if mix == 'pad_plus' else -1 if mix == 'pad_minus' else 0)
    acc = np.zeros((nrows, 128))
    ntap = taps + (1 if (mix == 'first_extra_tap' and first and p['extra']) else 0)
    for j in range(ntap):
        jw = min(j, taps - 1)                        # (mix: the tap the first filter does not have re-reads its last)
        if mix == 'tap_neighbour' and taps > 1:
            jw = j ^ 1 if (j ^ 1) < taps else j
        wh, wl = W[:, jw, 0, :], W[:, jw, 1, :]
        if mix == 'swap_w_planes':
            wh, wl = wl, wh
        ah, al = _shifted(xh, rows, j - pad, T), _shifted(xl, rows, j - pad, T)
        acc += ah @ (wh + wl).T if not absolute else ah @ wh.T + ah @ wl.T
        acc += al @ wh.T
        if mix == 'lolo':
            acc += al @ wl.T
    return acc


def ragged_pl(C):
    """Elements per plane of a ragged weight row: banks k = 1 .. C / 128 with k taps of 128 channels."""
    K = C // 128
    return 128 * K * (K + 1) // 2


def _acc_ragged(d, p, Bt, nrows, mix, absolute):
    C, T = d['C'], d['T']
    K, PL = C // 128, ragged_pl(C)
    X = d['X16'].astype(F64)
    xh, xl = X[:, :C], X[:, C:2 * C]
    W = np.asarray(Bt).astype(F64)
    if absolute:
        xh, xl, W = np.abs(xh), np.abs(xl), np.abs(W)
    rows = p['row0'] + np.arange(nrows)
    acc = np.zeros((nrows, 128))
    for k in range(1, K + 1):
        kx = k
        if mix == 'bank_neighbour':
            kx = k + 1 if k % 2 and k < K else (k - 1 if k % 2 == 0 else k)      # the activations of the neighbouring bank
        c0 = 128 * (kx - 1)
        for j in range(k):
            jw = j
            if mix == 'tap_neighbour' and k > 1:
                jw = j ^ 1 if (j ^ 1) < k else j
            o = (k * (k - 1) // 2 + jw) * 128
            wh, wl = W[:, o:o + 128], W[:, PL + o:PL + o + 128]
            if mix == 'half_neighbour':
                wh, wl = np.roll(wh, 64, axis=1), np.roll(wl, 64, axis=1)        # the two 64-channel halves of the row exchanged
            ah, al = _shifted(xh[:, c0:c0 + 128], rows, j - k // 2, T), _shifted(xl[:, c0:c0 + 128], rows, j - k // 2, T)
            acc += ah @ wh.T + ah @ wl.T + al @ wh.T
    return acc


def gemm16(d, mix=None, absolute=False, start=None):
    """-> flat float64 [nbuf]: `start` (default d['old'], else zeros) with everything the launch stores written over
    (or added to).  absolute=True returns sum |x| |w| |row_scale col_scale| in the stored elements instead (the
    magnitude the error bound of a real-valued case is taken from).  mix: a deliberate layout mix-up (CPU tests)."""
    if start is None:
        start = d['old'] if d.get('old') is not None else np.zeros(d['nbuf'])
    out = np.zeros(d['nbuf']) if absolute else np.array(start, dtype=F64)
    atomic = d.get('atomic_splits', 0) >= 1
    rs_all = None if d.get('row_scale') is None else np.asarray(d['row_scale'], F64)
    cs_all = None if d.get('col_scale') is None else np.asarray(d['col_scale'], F64)
    sh_all = None if d.get('col_shift') is None else np.asarray(d['col_shift'], F64)
    for p in d['pairs']:
        for Bt, taps, nrows, c_off, s_off, first in _filters(d, p):
            if nrows <= 0:
                continue
            if mix == 's_off_for_c_off':
                s_off = c_off % (len(cs_all) - 127) if atomic else (p['s_off0'] if first else p['s_off1'])
            acc = _acc_ragged(d, p, Bt, nrows, mix, absolute) if d['ragged'] else _acc_uniform(d, p, Bt, taps, nrows, first, mix, absolute)
            rows = p['row0'] + np.arange(nrows)
            rs = np.ones(nrows) if rs_all is None else rs_all[rows]
            cs = np.ones(128) if cs_all is None else cs_all[s_off:s_off + 128]
            sh = np.zeros(128) if sh_all is None else sh_all[s_off:s_off + 128]
            idx = np.arange(nrows)[:, None] * d['ldc'] + c_off + np.arange(128)[None, :]
            if absolute:
                out[idx] = acc * np.abs(rs)[:, None] * np.abs(cs)[None, :]
                continue
            v = acc * rs[:, None] * cs[None, :] + sh[None, :]
            if d.get('act', 0) == ACT_RELU:
                v = np.maximum(v, 0.0)
            if atomic or d.get('accumulate', 0):
                out[idx] += v
            else:
                out[idx] = v
    return out


def products_per_output(d, p, first):
    """n of the error bound: 3 plane products x taps x channels."""
    if d['ragged']:
        K = d['C'] // 128
        return 3 * 128 * K * (K + 1) // 2
    return 3 * (p['taps0'] + (0 if first else p['extra'])) * d['C']


def error_bound(d):
    """flat [nbuf]: (n + 3) * 2^-24 * sum |x| |w| * |row_scale col_scale| in every stored element, 0 elsewhere.  Any order
    of n float32 adds of exact products errs by at most (n - 1) u sum |x| |w| to first order, u = 2^-24; the two scale
    multiplications and the store's own rounding (no shift in the real-valued cases) are the other three u."""
    mag = gemm16(d, absolute=True)
    n = np.zeros(d['nbuf'])
    for p in d['pairs']:
        for Bt, taps, nrows, c_off, s_off, first in _filters(d, p):
            if nrows > 0:
                n[np.arange(nrows)[:, None] * d['ldc'] + c_off + np.arange(128)[None, :]] = products_per_output(d, p, first)
    return (n + 3) * 2.0 ** -24 * mag


# --------------------------------------------------------------------------------------------------------------------
# the operand kernels, bit for bit

def f32(a):
    return np.asarray(a, dtype=np.float32)


def pow2_scale(amax):
    """w16_scale: (s, 1 / s) for a float32 largest magnitude (NaN if the set held one).  s = 2^(14 - e), e the exponent
    of amax clamped at -100; 1 for zero, Inf and NaN."""
    bits = int(np.float32(amax).view(np.uint32))
    e = ((bits >> 23) & 255) - 127
    if not (amax > 0.0) or e >= 128:
        return 1.0, 1.0
    e = max(e, -100)
    return 2.0 ** (14 - e), 2.0 ** (e - 14)


def _absmax(v):
    """Largest magnitude of a float32 array, NaN if it holds a NaN (the kernels' NaN sticks)."""
    return np.float32(np.nan) if np.isnan(v).any() else np.float32(np.abs(v).max(initial=0.0))


def prologue(X, scale, shift, relu):
    """pro_val: fmaf(x, scale, shift) rounded once, then relu as fmaxf(v, 0) (which turns a NaN into 0)."""
    X = f32(X)
    if scale is None and shift is None and not relu:
        return X
    sc = 1.0 if scale is None else np.asarray(scale, F64)[None, :]
    sh = 0.0 if shift is None else np.asarray(shift, F64)[None, :]
    with np.errstate(all='ignore'):
        v = f32(X.astype(F64) * sc + sh)
        return f32(np.fmax(v, np.float32(0.0))) if relu else v


def pool_same(v, T):
    """max-pool(2, 1, same) along time inside each window of T rows: frame t takes fmaxf(v[t], v[t + 1]), the last its own."""
    M, C = v.shape
    w = v.reshape(M // T, T, C)
    out = w.copy()
    out[:, :-1] = np.fmax(w[:, :-1], w[:, 1:])
    return out.reshape(M, C)


def split_hi_lo(xs):
    """float32 -> (hi, lo) float16."""
    with np.errstate(all='ignore'):
        xs = f32(xs)
        hi = xs.astype(np.float16)
        lo = f32(xs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split16(X, C, T, scale=None, shift=None, relu=0, pool=0):
    """X [M, >= C] float32 -> (out16 [M, 2C] float16, row_scale [M] float32)."""
    M = X.shape[0]
    v = prologue(np.asarray(X)[:, :C], scale, shift, relu)
    s = np.empty(M)
    rs = np.empty(M, np.float32)
    for w in range(M // T):
        sw, rw = pow2_scale(_absmax(v[w * T:(w + 1) * T]))
        s[w * T:(w + 1) * T], rs[w * T:(w + 1) * T] = sw, rw
    if pool:
        v = pool_same(v, T)
    with np.errstate(all='ignore'):
        xs = f32(v.astype(F64) * s[:, None])
    hi, lo = split_hi_lo(xs)
    return np.concatenate([hi, lo], axis=1), rs


def transpose_split16(X, C, T, shift0=0, n_shifts=1, scale=None, shift=None, relu=0, pool=0, shift_bias=0):
    """X [M, >= C] float32 -> (out16 [n_shifts * C, 2M] float16, row_scale [n_shifts * C] float32).
    shift_bias: the deliberate off-by-one of the CPU tests."""
    M = X.shape[0]
    v = prologue(np.asarray(X)[:, :C], scale, shift, relu)
    sc = np.array([pow2_scale(_absmax(v[:, c])) for c in range(C)])
    if pool:
        v = pool_same(v, T)
    with np.errstate(all='ignore'):
        xs = f32(v.astype(F64) * sc[None, :, 0])
    hi, lo = split_hi_lo(xs)
    out = np.zeros((n_shifts * C, 2 * M), np.float16)
    m = np.arange(M)
    for si in range(n_shifts):
        s = shift0 + si + shift_bias
        ok = ((m % T) + s >= 0) & ((m % T) + s < T)
        src = np.clip(m + s, 0, M - 1)
        out[si * C:(si + 1) * C, :M] = np.where(ok[None, :], hi[src].T, np.float16(0))
        out[si * C:(si + 1) * C, M:] = np.where(ok[None, :], lo[src].T, np.float16(0))
    return out, np.tile(sc[:, 1].astype(np.float32), n_shifts)


def weights16(items, bufs, n_groups, mode_as=None):
    """items: dicts(src [k, cin, cout] float32, dst (key of bufs: a flat float16 array), k, cin, cout, mode, row_len,
    tap_stride, plane_stride, base, group, scale_dst (key of bufs: float32 array, or None), scale_off, scale_n).
    Writes into copies of bufs and returns them.  mode_as: read every item's mode as this one (CPU tests)."""
    bufs = {k: v.copy() for k, v in bufs.items()}
    gmax = [np.float32(0.0)] * n_groups
    for it in items:
        a, g = _absmax(f32(it['src'])), it['group']
        gmax[g] = np.float32(np.nan) if np.isnan(a) or np.isnan(gmax[g]) else max(gmax[g], a)
    for it in items:
        s, rs = pow2_scale(gmax[it['group']])
        if it.get('scale_dst') is not None:
            o = it.get('scale_off', 0)
            bufs[it['scale_dst']][o:o + it['scale_n']] = rs
        k, cin, cout = it['k'], it['cin'], it['cout']
        with np.errstate(all='ignore'):
            hi, lo = split_hi_lo(f32(f32(it['src']).astype(F64) * s))
        dst = bufs[it['dst']]
        j, c, o = np.meshgrid(np.arange(k), np.arange(cin), np.arange(cout), indexing='ij')
        mode = it['mode'] if mode_as is None else mode_as
        if mode == 0:
            at = o * it['row_len'] + it['base'] + j * it['tap_stride'] + c
        else:
            at = c * it['row_len'] + it['base'] + (k - 1 - j) * it['tap_stride'] + o
        dst[at.ravel()] = hi.ravel()
        dst[at.ravel() + it['plane_stride']] = lo.ravel()
    return bufs


# --------------------------------------------------------------------------------------------------------------------
# the launcher's host rules

def choose_ksplit(max_rows, n_pairs, kslabs):
    """vc_gemm16.hip choose_ksplit:
        if (n_pairs != 1) return 1;
        int s = 256 / ntm;  if (s > MAX_SPLIT) s = MAX_SPLIT;  if (s > kslabs / 4) s = kslabs / 4;  return s < 2 ? 1 : s;"""
    ntm = (max_rows + BM - 1) // BM
    if n_pairs != 1:
        return 1
    s = min(256 // ntm, MAX_SPLIT, kslabs // 4)
    return 1 if s < 2 else s


def split_points(kslabs, nsl, ks, ragged):
    """vc_gemm16.hip, the split_cs loop:
        for (c = 0; c < kslabs && nxt < ks; ++c) { run += ragged ? ((c % nsl) >> 1) + 1 : 1;
                                                   if (run * ks >= total * nxt) split_cs[nxt++] = c + 1; }"""
    wt = [(((c % nsl) >> 1) + 1) if ragged else 1 for c in range(kslabs)]
    total, run, nxt, cs = sum(wt), 0, 1, [0]
    for c in range(kslabs):
        if nxt >= ks:
            break
        run += wt[c]
        if run * ks >= total * nxt:
            cs.append(c + 1)
            nxt += 1
    while len(cs) <= ks:
        cs.append(kslabs)
    cs[ks] = kslabs
    return cs


def pair16_map(ntm):
    """vc_gemm16.hip, n_pairs == 16: XCD x takes half `x & 1` of the row tiles (h0 = (ntm + 1) / 2 first) of the pairs
    15 - {s4, 7 - s4, 8 + s4, 15 - s4}, s4 = x >> 1.  -> (blocks, [(pair, row tile) or None per block])."""
    h0 = (ntm + 1) // 2
    seg, max_slots = [], 0
    for x in range(8):
        s4, half = x >> 1, x & 1
        ent = [(15 - r, h0 if half else 0, ntm - h0 if half else h0) for r in (s4, 7 - s4, 8 + s4, 15 - s4)]
        seg.append(ent)
        max_slots = max(max_slots, sum(e[2] for e in ent))
    work = []
    for b in range(8 * max_slots):
        x, slot, got = b & 7, b >> 3, None
        for pair, first, cnt in seg[x]:
            if got is None and slot < cnt:
                got = (pair, first + slot)
            slot -= cnt
        work.append(got)
    return 8 * max_slots, work


def launch_plan(d, forced=-1, workspace_bytes=0):
    """What vc_gemm16 launches for descriptor d under option gemm16_split = forced with that much workspace:
    dict(form, ks, split_map, split_cs, blocks, ntm, idle) -- idle: workgroups that return without a tile."""
    nsl = d['C'] >> 6
    kslabs = 3 * nsl
    max_rows = max(max(pair_rows(d, p)) for p in d['pairs'])
    ntm = (max_rows + BM - 1) // BM
    n_pairs = len(d['pairs'])
    zs = d.get('atomic_splits', 0)
    if zs >= 1:
        return dict(form='atomic', ks=zs, split_map=0, split_cs=[kslabs * i // zs for i in range(zs + 1)], blocks=ntm * n_pairs * zs,
                    ntm=ntm, idle=0)
    ks, split_map = choose_ksplit(max_rows, n_pairs, kslabs), 0
    # if (forced >= 1 && n_pairs == 1) { want = forced & 15; if (want >= 1 && want <= MAX_SPLIT && want * 2 <= kslabs) { ks = want;
    #     split_map = (forced >> 4) == 1 && (8 % want) == 0 && want > 1; } }
    if forced >= 1 and n_pairs == 1:
        want = forced & 15
        if 1 <= want <= MAX_SPLIT and want * 2 <= kslabs:
            ks = want
            split_map = int((forced >> 4) == 1 and 8 % want == 0 and want > 1)
    # if (ks > 1 && (!workspace || workspace_bytes < tick_bytes(ntm) + ntm * ks * 262144)) ks = 1;
    if ks > 1 and workspace_bytes < -(-ntm * 4 // 256) * 256 + ntm * ks * 262144:
        ks = 1
    if ks > 1:
        blocks = 8 * (-(-ntm // (8 // ks))) if split_map else ntm * ks
        return dict(form='split', ks=ks, split_map=split_map, split_cs=split_points(kslabs, nsl, ks, bool(d['ragged'])), blocks=blocks,
                    ntm=ntm, idle=blocks - ntm * ks)
    if n_pairs == 16:
        blocks, work = pair16_map(ntm)
        return dict(form='xcd16', ks=1, split_map=0, split_cs=[0, kslabs], blocks=blocks, ntm=ntm, idle=sum(w is None for w in work))
    return dict(form='plain', ks=1, split_map=0, split_cs=[0, kslabs], blocks=ntm * n_pairs, ntm=ntm, idle=0)


def workspace_bytes(M, C, n_pairs):
    """vc_gemm16_workspace_bytes."""
    if M <= 0 or C <= 0 or C & 63 or n_pairs != 1 or 3 * (C >> 6) < 8:
        return 0
    ntm = (M + BM - 1) // BM
    return -(-ntm * 4 // 256) * 256 + ntm * MAX_SPLIT * 262144


def split16_tl_seg(M, C, T):
    """vc_split16:  tl = 4; while ((1 << tl) < C / 4 && tl < 8) ++tl;  while (C % (4 << tl)) --tl;
                    seg = 1024 / nwin, clamped to 1 .. T.   -> (tl, groups per thread, seg)"""
    tl = 4
    while (1 << tl) < C // 4 and tl < 8:
        tl += 1
    while C % (4 << tl):
        tl -= 1
    seg = min(max(1024 // (M // T), 1), T)
    return tl, C // (4 << tl), seg
