"""Spectral mapping on the MI355X: every launch of csrc/vc_mapping.hip alone through the C ABI against tests/mapping_ref.py
inside guarded, NaN-filled buffers; batch independence, graph replay and the absence of host synchronisation; and the method
end to end on a small synthetic parallel corpus.

vc_jd_prepare_f32, vc_jd_update_f32 and vc_mlpg_f32 are float64 rounded once and are compared bit for bit (the two constants
of prepare that take a logarithm: within one float32 unit in the last place of the restatement's, the distance a float64
log that differs in its last bits can move a rounding).  vc_jd_accumulate_f32 and vc_jd_map_f32 are held to the bounds that
mapping_ref derives; tests/test_mapping_cpu.py holds the float32 twin to half of each of them on the same inputs.

Restatement's end-to-end figures (mapping_ref.e2e_restatement, float64; 8 + 2 sentences, 24 cepstra, 8 components, 10
iterations): held-out MCD 16.431 dB unconverted, 0.933 dB for the converted cepstra, 6.469 dB for the filtered waveform; its
float32 twin differs by less than 1e-6 dB, so the margin is the floor of 0.05 dB."""
import numpy as np
import pytest
import torch

from conftest import poison_gpu_state
import diff_ref
import mapping_cases as mc
import mapping_ref as mr

pytestmark = pytest.mark.gpu

BAND = 1024                     # guard elements on either side of every buffer
U = mr.U
E2E_REF = dict(before=16.431, cep=0.933, wav=6.469)
E2E_MARGIN = 0.05               # max(3 x the restatement's float32-to-float64 gap, 0.05 dB); the gap is below 1e-6 dB


@pytest.fixture(autouse=True)
def _poisoned():
    poison_gpu_state()


class Guarded:
    """n elements of ``dtype`` inside a larger device buffer whose bands hold a sentinel; .t is the inner view, NaN-filled
    (integers: the sentinel) unless ``host`` is given."""
    SENT = {torch.float32: -98765.4375, torch.float64: -98765.4375, torch.int32: -1234567, torch.uint8: 0xA5}

    def __init__(self, n, dtype=torch.float32, host=None):
        self.sent = self.SENT[dtype]
        self.full = torch.full((n + 2 * BAND,), self.sent, dtype=dtype, device='cuda')
        self.t = self.full[BAND:BAND + n]
        if host is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).to(dtype))
        elif dtype.is_floating_point:
            self.t.fill_(float('nan'))

    def check(self, what):
        assert bool((self.full[:BAND] == self.sent).all()) and bool((self.full[-BAND:] == self.sent).all()), \
            'sentinel band overwritten around ' + what

    def numpy(self):
        return self.t.cpu().numpy()


def _lib():
    import _vc
    return _vc.lib()


def _ok(rc):
    import _vc
    _vc.check(rc)


def _st():
    import _vc
    return _vc.current_stream()


def _p(g):
    import _vc
    return None if g is None else _vc.ptr(g.t)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _checked(bufs):
    torch.cuda.synchronize()
    for name, g in bufs.items():
        if g is not None:
            g.check(name)


def _measured(what, got, want, bound):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    ratio = np.abs(got - want) / (bound + 1e-300)
    r = float(ratio.max()) if ratio.size else 0.0
    print('MEASURED %s: worst error / bound %.3f' % (what, r))
    assert r <= 1.0, what
    return r


# ------------------------------------------------------------------------------------------------------------- the launches
def run_prepare(model):
    M, D = model['mu_x'].shape
    ins = {k: Guarded(model[k].size, host=model[k]) for k in mr.FIELDS}
    tab = Guarded(mr.table_floats(M, D))
    _ok(_lib().vc_jd_prepare_f32(*(_p(ins[k]) for k in mr.FIELDS), M, D, _p(tab), _st()))
    _checked(dict(ins, table=tab))
    return tab


def run_accumulate(model, fa, fb, la, lb, path, plen, tab=None):
    M, D = model['mu_x'].shape
    tab = tab or run_prepare(model)
    B, Fa, Fb = fa.shape[0], fa.shape[1], fb.shape[1]
    bufs = dict(fa=Guarded(fa.size, host=fa), fb=Guarded(fb.size, host=fb), la=Guarded(B, torch.int32, la), lb=Guarded(B, torch.int32, lb),
                path=None if path is None else Guarded(path.size, torch.int32, path),
                plen=None if path is None else Guarded(B, torch.int32, plen),
                N=Guarded(M, torch.float64), S=Guarded(5 * M * D, torch.float64), L=Guarded(2, torch.float64),
                ws=Guarded(mr.workspace_size(M, D) // 8, torch.float64))
    _ok(_lib().vc_jd_accumulate_f32(_p(bufs['fa']), _p(bufs['fb']), _p(bufs['la']), _p(bufs['lb']), _p(bufs['path']), _p(bufs['plen']),
                                    B, Fa, Fb, 0 if path is None else path.shape[1], D, _p(tab), M, _p(bufs['N']), _p(bufs['S']),
                                    _p(bufs['L']), _p(bufs['ws']), mr.workspace_size(M, D), _st()))
    _checked(bufs)
    return dict(N=bufs['N'].numpy(), S=bufs['S'].numpy().reshape(5, M, D), L=bufs['L'].numpy())


def run_update(N, S, model, fx, fy, rho_max, min_count):
    M, D = model['mu_x'].shape
    ins = {k: Guarded(model[k].size, host=model[k]) for k in mr.FIELDS[1:]}
    bufs = dict(N=Guarded(M, torch.float64, N), S=Guarded(S.size, torch.float64, S), fx=Guarded(D, host=fx), fy=Guarded(D, host=fy))
    outs = {k: Guarded(M if k == 'w' else M * D) for k in mr.FIELDS}
    _ok(_lib().vc_jd_update_f32(_p(bufs['N']), _p(bufs['S']), M, D, *(_p(ins[k]) for k in mr.FIELDS[1:]), _p(bufs['fx']), _p(bufs['fy']),
                                rho_max, min_count, *(_p(outs[k]) for k in mr.FIELDS), _st()))
    _checked(dict(bufs, **{'out_' + k: v for k, v in outs.items()}))
    return {k: outs[k].numpy().reshape(model[k].shape) for k in mr.FIELDS}


def run_map(model, feat, lens, mixture, tab=None, mmse=True):
    M, D = model['mu_x'].shape
    tab = tab or run_prepare(model)
    B, F, _ = feat.shape
    bufs = dict(feat=Guarded(feat.size, host=feat), lens=Guarded(B, torch.int32, lens), P=Guarded(feat.size), R=Guarded(feat.size),
                E=Guarded(feat.size) if mmse else None, best=Guarded(B * F, torch.int32))
    _ok(_lib().vc_jd_map_f32(_p(bufs['feat']), _p(bufs['lens']), B, F, D, _p(tab), M, mixture, _p(bufs['P']), _p(bufs['R']), _p(bufs['E']),
                             _p(bufs['best']), _st()))
    _checked(bufs)
    out = {k: bufs[k].numpy().reshape(B, F, D) for k in ('P', 'R')}
    out['E'] = bufs['E'].numpy().reshape(B, F, D) if mmse else None
    out['best'] = bufs['best'].numpy().reshape(B, F)
    return out


def run_mlpg(P, R, lens):
    B, F, D = P.shape
    n = D // 2
    need = mr.mlpg_workspace_size(B, F, n)
    bufs = dict(P=Guarded(P.size, host=P), R=Guarded(R.size, host=R), lens=Guarded(B, torch.int32, lens), y=Guarded(B * F * n),
                flags=Guarded(B, torch.int32), ws=Guarded(need // 8, torch.float64))
    _ok(_lib().vc_mlpg_f32(_p(bufs['P']), _p(bufs['R']), _p(bufs['lens']), B, F, n, _p(bufs['y']), _p(bufs['flags']), _p(bufs['ws']), need,
                           _st()))
    _checked(bufs)
    return bufs['y'].numpy().reshape(B, F, n), bufs['flags'].numpy()


# ----------------------------------------------------------------------------------------------------------------- prepare
@pytest.mark.parametrize('M,D', mc.JD_SHAPES)
def test_prepare_bit_for_bit(M, D):
    model = mr.random_model(M, D, seed=M + D)
    got = run_prepare(model).numpy()
    T = mr.prepare(model)
    want = mr.table_layout(T)
    n = M * D
    logs = slice(6 * n, 6 * n + 2 * M)
    exact = np.ones(len(want), bool)
    exact[logs] = False
    assert _same_bits(got[exact], want[exact])
    ulp = np.spacing(np.abs(want[logs]))
    d = np.abs(got[logs].astype(np.float64) - want[logs].astype(np.float64)) / ulp
    print('MEASURED vc_jd_prepare_f32 M=%d D=%d: c, cx at most %.1f float32 ulp from the restatement, %d of %d not bit-identical'
          % (M, D, d.max(), int((d > 0).sum()), 2 * M))
    assert d.max() <= 1.0


# ------------------------------------------------------------------------------------------------------------------ update
@pytest.mark.parametrize('M,D', mc.JD_SHAPES)
def test_update_bit_for_bit(M, D):
    """Statistics of a float64 E-step on the case's cells; component 0 is starved, the correlation clamp is reached (rho_max
    0.3) and a floor too (floors at the global variance)."""
    model, fa, fb, la, lb, path, plen = mc.acc_case(M, D)
    st = mr.accumulate(*mr.gather(fa, fb, la, lb, path, plen), model)
    N, S = st['N'].copy(), st['S'].copy()
    N[0] = 0.25
    fx, fy = np.full(D, 1.0, np.float32), np.full(D, 1e-3, np.float32)
    want = mr.update(N, S, model, fx, fy, 0.3, 1.0)
    got = run_update(N, S, model, fx, fy, 0.3, 1.0)
    for k in mr.FIELDS:
        assert _same_bits(got[k], want[k]), k
    if M > 1:
        assert np.array_equal(got['mu_x'][0], model['mu_x'][0]) and (got['var_x'][1:] == 1.0).any()
        rho = got['cov_xy'][1:] / np.sqrt(got['var_x'][1:].astype(np.float64) * got['var_y'][1:])
        assert np.abs(rho).max() > 0.29


# -------------------------------------------------------------------------------------------------------------- accumulate
@pytest.mark.parametrize('with_path', [True, False])
@pytest.mark.parametrize('M,D', mc.JD_SHAPES)
def test_accumulate_two_delta_rule(M, D, with_path):
    model, fa, fb, la, lb, path, plen = mc.acc_case(M, D, with_path)
    want = mr.accumulate(*mr.gather(fa, fb, la, lb, path, plen), model)
    got = run_accumulate(model, fa, fb, la, lb, path, plen)
    again = run_accumulate(model, fa, fb, la, lb, path, plen)
    for k in ('N', 'S', 'L'):
        assert _same_bits(got[k], again[k]), k + ': not bit-identical from run to run'
    d = want['delta']
    tag = 'vc_jd_accumulate_f32 M=%d D=%d %s' % (M, D, 'path' if with_path else 'NULL path')
    assert got['L'][1] == want['L'][1]
    _measured(tag + ' N', got['N'], want['N'], 2 * d * want['N'])
    _measured(tag + ' S', got['S'], want['S'], 2 * d * want['A'])
    _measured(tag + ' L', got['L'][:1], want['L'][:1], d * want['L'][1])


def test_accumulate_per_cell_log_likelihood():
    """One cell per call (a path of one cell): L is that cell's ll, held to the per-cell bound."""
    M, D = 65, 48
    model, fa, fb, la, lb, _, _ = mc.acc_case(M, D, False)
    tab = run_prepare(model)
    worst = 0.0
    for i, j in ((0, 0), (69, 49), (31, 32), (5, 40)):
        path = np.array([[[i, j]], [[0, 0]], [[0, 0]]], np.int32)
        got = run_accumulate(model, fa, fb, la, lb, path, np.array([1, 0, 0], np.int32), tab)
        ll, E, _ = mr.joint_ll(fa[0, i][None], fb[0, j][None], model)
        assert got['L'][1] == 1.0
        worst = max(worst, abs(got['L'][0] - ll[0]) / mr.cell_bound(D, M, E)[0])
    print('MEASURED vc_jd_accumulate_f32 per-cell ll: worst error / bound %.3f' % worst)
    assert worst <= 1.0


# --------------------------------------------------------------------------------------------------------------------- map
@pytest.mark.parametrize('mixture', ['soft', 'best'])
@pytest.mark.parametrize('M,D', mc.JD_SHAPES)
def test_map_against_float64_and_alone(M, D, mixture):
    model, feat, lens = mc.map_case(M, D)
    tab = run_prepare(model)
    got = run_map(model, feat, lens, mc_mix(mixture), tab)
    tag = 'vc_jd_map_f32 %s M=%d D=%d' % (mixture, M, D)
    worst = 0.0
    for b, l in enumerate(lens):
        for k in ('P', 'R', 'E'):
            assert not _bits(got[k][b, l:]).any(), (k, b)              # +0 from the length on
        assert not got['best'][b, l:].any()
        if l == 0:
            continue
        P, R, E, best, bd = mr.map_stats(feat[b, :l], model, mixture)
        assert np.array_equal(got['best'][b, :l], best)
        worst = max(worst, _measured('%s b=%d P' % (tag, b), got['P'][b, :l], P, bd['P']),
                    _measured('%s b=%d R' % (tag, b), got['R'][b, :l], R, bd['R']),
                    _measured('%s b=%d mmse' % (tag, b), got['E'][b, :l], E, bd['mmse']))
        alone = run_map(model, feat[b:b + 1, :l].copy(), [l], mc_mix(mixture), tab)
        for k in ('P', 'R', 'E', 'best'):
            assert np.array_equal(_bits(alone[k][0]), _bits(got[k][b, :l])), (k, b, 'alone differs from the batch')
    print('MEASURED %s: worst of all rows %.3f' % (tag, worst))
    no_e = run_map(model, feat, lens, mc_mix(mixture), tab, mmse=False)
    assert _same_bits(no_e['P'], got['P']) and _same_bits(no_e['R'], got['R'])


def mc_mix(mixture):
    return {'soft': 0, 'best': 1}[mixture]


# -------------------------------------------------------------------------------------------------------------------- mlpg
@pytest.mark.parametrize('n', mc.MLPG_COEF)
def test_mlpg_bit_for_bit(n):
    P, R = mc.mlpg_case(n)
    lens = list(mc.MLPG_LENS)
    y, flags = run_mlpg(P, R, lens)
    assert not flags.any()
    for b, l in enumerate(lens):
        want, flag = mr.mlpg(P[b], R[b], l)
        assert flag == 0 and _same_bits(y[b], want), (n, b, l, np.abs(y[b] - want).max())
        if l:
            alone, f1 = run_mlpg(P[b:b + 1, :l].copy(), R[b:b + 1, :l].copy(), [l])
            assert _same_bits(alone[0], y[b, :l]) and not f1.any()
    # lengths beyond max_frames and below 0 are clamped
    full_P, full_R = np.where(np.isnan(P[-1:]), np.float32(1), P[-1:]), np.nan_to_num(R[-1:])
    y2, _ = run_mlpg(full_P, full_R, [10 ** 6])
    assert _same_bits(y2[0], mr.mlpg(full_P[0], full_R[0], full_P.shape[1])[0])
    y3, f3 = run_mlpg(P[-1:], R[-1:], [-3])
    assert not _bits(y3).any() and not f3.any()


def test_mlpg_flag_and_fallback():
    P, R = mc.mlpg_case(2, [9, 9])
    P[0, 3, 0] = -40.0
    y, flags = run_mlpg(P, R, [9, 9])
    assert flags.tolist() == [1, 0]
    for b in range(2):
        want, flag = mr.mlpg(P[b], R[b], 9)
        assert flag == flags[b] and _same_bits(y[b], want)
    assert _same_bits(y[0, :9, 0], (R[0, :9, 0].astype(np.float64) / P[0, :9, 0].astype(np.float64)).astype(np.float32))


# -------------------------------------------------------------------------------------------------------------------- gain
@pytest.mark.parametrize('n,F', mc.GAIN_CASES)
def test_cep_gain_against_the_float32_twin(n, F):
    import evaluation
    import mapping
    cy, cx, nf = mc.gain_case(n, F)
    dct = evaluation.dct_rows(80, n, 1)
    i0, w = mapping.gain_tables(mc.CFG)
    scale = 3.0 * mapping.db_scale(mc.CFG)                           # (x 3: some bins reach both clamps)
    B, Fm, nb = cy.shape[0], cy.shape[1], len(i0)
    bufs = dict(cy=Guarded(cy.size, host=cy), cx=Guarded(cx.size, host=cx), nf=Guarded(B, torch.int32, nf), dct=Guarded(dct.size, host=dct),
                i0=Guarded(nb, torch.int32, i0), w=Guarded(nb, host=w), g=Guarded(B * Fm * nb))
    _ok(_lib().vc_cep_gain_f32(_p(bufs['cy']), _p(bufs['cx']), _p(bufs['nf']), B, Fm, n, _p(bufs['dct']), 80, _p(bufs['i0']), _p(bufs['w']), nb,
                               0.75, scale, 6.0, 9.0, _p(bufs['g']), _st()))
    _checked(bufs)
    got = bufs['g'].numpy().reshape(B, Fm, nb)
    s32 = mr.cep_gain_s(cy, cx, nf, dct, i0, w, 0.75, scale, 6.0, 9.0, np.float32)
    want = diff_ref.gain_from_s(s32)
    live = ~np.isnan(s32)
    assert not _bits(got[~live]).any()
    if live.any():
        r = np.abs(got[live] - want[live]) / (diff_ref.exp2_rel_bound() * want[live])
        print('MEASURED vc_cep_gain_f32 n=%d F=%d: worst error / bound %.3f; clamped low %d, high %d of %d' % (
            n, F, r.max(), int((s32[live] == -9).sum()), int((s32[live] == 6).sum()), int(live.sum())))
        assert r.max() <= 1.0


# ----------------------------------------------------------------------------------------------- graph, batch, sync, python
def _device_corpus():
    xs, ys = mr.cepstral_corpus()
    X, lens = mr.batch(xs, pad=2)
    Y, _ = mr.batch(ys, pad=2)
    return X, Y, lens


def test_graph_replay_of_every_launch():
    """prepare, accumulate (both launches), update, map, mlpg and the gain captured once, replayed with other features,
    lengths and paths copied into the static tensors: bit-identical to eager calls on the same inputs."""
    import evaluation
    import mapping
    from test_graph_replay_gpu import _capture, _free, _same
    X, Y, lens = _device_corpus()
    fa, fb = mr.features_batch(X, lens), mr.features_batch(Y, lens)
    B, F, D = fa.shape
    M = 8
    m0 = mr.random_model(M, D, seed=3, spread=0.5)
    d_dct = torch.from_numpy(evaluation.dct_rows(80, D // 2, 1)).cuda()
    d_i0, d_w = (torch.from_numpy(a).cuda() for a in mapping.gain_tables(mc.CFG))
    floor = torch.full((D,), 1e-3, device='cuda')

    def inputs(k):
        rng = np.random.RandomState(50 + k)
        la = np.array([max(l - 3 * k - b, 1) for b, l in enumerate(lens)], np.int32)
        path = np.full((B, 2 * F - 1, 2), -1, np.int32)
        plen = np.zeros(B, np.int32)
        for b in range(B):
            c = mc.monotone_path(int(la[b]), lens[b], rng)
            path[b, :len(c)], plen[b] = c, len(c)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return [t(np.roll(fa, k, 0)), t(fb), t(la), t(np.array(lens, np.int32)), t(path), t(plen)] + \
               [t(m0[f] * np.float32(1 + 0.01 * k) if f.startswith('var') else m0[f]) for f in mr.FIELDS]

    def chain(a, b, la, lb, path, plen, *model):
        model = mapping.JDGMM(*model)
        tab = mapping._prepare_launch(model)
        st = mapping._accumulate_launch(a, b, la, lb, path, plen, tab, M)
        new = mapping._update_launch(st, model, floor, floor, 0.99, 1.0)
        r = mapping._map_launch(a, la, tab, M, 0)
        y = mapping._mlpg_launch(r.P, r.R, la)
        g = mapping._gain_launch(y.y, a[:, :, :D // 2].contiguous(), la, d_dct, d_i0, d_w, 1.0, 50.0, 20.0, 30.0)
        return (tab, st.N, st.S, st.L) + tuple(new) + tuple(r) + (y.y, y.flags, g)

    static = inputs(0)
    g, outs = _capture(lambda: chain(*static))
    try:
        for k in range(1, 3):
            new = inputs(k)
            for s, t in zip(static, new):
                s.copy_(t)
            g.replay()
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(outs, chain(*new))):
                _same(a, b, 'replay %d output %d' % (k, i))
            assert torch.isfinite(outs[-1]).all() and float(outs[1].sum()) > 0
    finally:
        _free(g)


def test_fit_equals_the_restatement_and_nothing_waits():
    """mapping.fit on the cepstral corpus against mapping_ref.fit (float64) under the same arguments.  EM carries a rounding
    of one iteration into the next, so no forward bound follows from the per-cell one; the yardstick is the restatement's own
    float32 twin, as for the end-to-end figures: every parameter and the trace within 4 x the twin's distance from float64
    (and one float32 rounding of the value).  fit and convert_cepstra_batch run under set_sync_debug_mode('error')."""
    import mapping
    X, Y, lens = _device_corpus()
    fa, fb = mr.features_batch(X, lens), mr.features_batch(Y, lens)
    want, trace = mr.fit(fa[:8], fb[:8], lens[:8], lens[:8], n_components=8, n_iter=6)
    twin, trace32 = mr.fit(fa[:8], fb[:8], lens[:8], lens[:8], n_components=8, n_iter=6, dtype=np.float32)
    d_fa, d_fb, d_X = (torch.from_numpy(a).cuda() for a in (fa[:8], fb[:8], X))
    mapping.fit(d_fa, lens[:8], d_fb, lens[:8], n_components=8, n_iter=1)          # warm-up: allocations, the library
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        model, tr = mapping.fit(d_fa, lens[:8], d_fb, lens[:8], n_components=8, n_iter=6)
        conv = mapping.convert_cepstra_batch(model, d_X, lens)
        conv_mmse = mapping.convert_cepstra_batch(model, d_X, lens, mixture='best', mlpg=False)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    tr = tr.cpu().numpy()
    print('MEASURED mapping.fit trace: device %s, restatement %s' % (np.round(tr, 5).tolist(), np.round(trace, 5).tolist()))
    assert np.abs(tr - trace).max() <= 4 * np.abs(trace32 - trace).max() + 2 * U * np.abs(trace).max()
    for k, t in zip(mr.FIELDS, model):
        got = t.cpu().numpy().astype(np.float64)
        gap = np.abs(twin[k].astype(np.float64) - want[k]).max()
        print('MEASURED mapping.fit %s: device %.3e from float64, the twin %.3e' % (k, np.abs(got - want[k]).max(), gap))
        assert np.abs(got - want[k]).max() <= 4 * gap + 2 * U * np.abs(want[k]).max(), k
    conv, conv_mmse = conv.cpu().numpy(), conv_mmse.cpu().numpy()
    e0 = e1 = 0.0
    for b in (8, 9):
        F = lens[b]
        e0 += ((X[b, :F] - Y[b, :F]) ** 2).sum()
        e1 += ((conv[b, :F] - Y[b, :F]) ** 2).sum()
        assert not conv[b, F:].any() and not conv_mmse[b, F:].any() and np.isfinite(conv_mmse).all()
    assert e1 < e0


@pytest.fixture(scope='module')
def wavs():
    src, tgt = mr.wav_corpus(mr.E2E['n_fit'] + mr.E2E['n_held'])
    return mr.wav_batch(src), mr.wav_batch(tgt)


def test_end_to_end_on_the_parallel_corpus(wavs):
    """fit_wav on 8 parallel sentences, convert_gmm_diff_batch on the 2 held out; the device's held-out MCD (mcd_wav_batch
    against the target) of the converted cepstra and of the filtered waveform: each below the unconverted MCD and equal to
    the float64 restatement's within E2E_MARGIN.  convert_gmm_diff_batch runs under set_sync_debug_mode('error')."""
    import conversion
    import evaluation
    import mapping
    (S, ls), (T, lt) = wavs
    nf, p = mr.E2E['n_fit'], mr.E2E
    model, trace = mapping.fit_wav(S[:nf], ls[:nf], T[:nf], lt[:nf], mc.CFG, n_coef=p['n_coef'], n_components=p['n_components'],
                                   n_iter=p['n_iter'])
    d_S = torch.from_numpy(S[nf:]).cuda()
    conversion.convert_gmm_diff_batch(model, d_S, ls[nf:], mc.CFG)                  # warm-up: plans, tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = conversion.convert_gmm_diff_batch(model, d_S, ls[nf:], mc.CFG)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    hop = mc.CFG['hop_length']
    assert r.n_frames == [1 + l // hop for l in ls[nf:]] and r.n_samples == [hop * (l // hop) for l in ls[nf:]]
    before = float(evaluation.mcd_wav_batch(S[nf:], ls[nf:], T[nf:], lt[nf:], mc.CFG).mcd.mean())
    wav = float(evaluation.mcd_wav_batch(r.y_wav_pred, r.n_samples, T[nf:], lt[nf:], mc.CFG).mcd.mean())
    # the converted cepstra against the target's: the same DTW on cepstra
    d_T = torch.from_numpy(T[nf:]).cuda()
    d_lt, = evaluation._upload_lens(lt[nf:])
    cb = evaluation._cepstra_launch(evaluation._mel_launch(d_T, d_lt, mc.CFG), p['n_coef'], 1)
    scale = 1.0 / (4.0 * mc.CFG['M_dB_norm_factor'])
    cep = float(evaluation.dtw_batch(r.cep_pred, cb, r.n_frames, [1 + l // hop for l in lt[nf:]], scale=scale).mcd.mean())
    print('MEASURED end to end: held-out MCD %.3f dB unconverted, %.3f dB converted cepstra (restatement %.3f), %.3f dB filtered '
          'waveform (restatement %.3f); trace %.3f -> %.3f' % (before, cep, E2E_REF['cep'], wav, E2E_REF['wav'], float(trace[0]),
                                                              float(trace[-1])))
    assert cep < before and wav < before
    assert abs(cep - E2E_REF['cep']) <= E2E_MARGIN and abs(wav - E2E_REF['wav']) <= E2E_MARGIN
    # alpha = 0 returns the source through the filter: gain 1 on every used frame
    r0 = conversion.convert_gmm_diff_batch(model, d_S, ls[nf:], mc.CFG, alpha=0.0)
    assert bool((r0.gain[0, :r0.n_frames[0]] == 1.0).all()) and not bool(r0.gain[1, r0.n_frames[1]:].any())


def test_realignment_resampling_and_denoising_paths(wavs):
    """fit_wav with one realignment (DTW of the converted source against the target, then a second fit), and
    convert_gmm_diff_batch on 8 kHz input with denoise and an 8 kHz output: the launches of the other modules in front of and
    behind the mapping.  Finite, the stated frame and sample counts, zeros beyond them, and the realigned model still
    converts the held-out cepstra towards the target."""
    import audio_lib
    import conversion
    import evaluation
    import mapping
    (S, ls), (T, lt) = wavs
    nf, hop = 4, mc.CFG['hop_length']
    model, trace = mapping.fit_wav(S[:nf], ls[:nf], T[:nf], lt[:nf], mc.CFG, n_realign=1, n_components=4, n_iter=4)
    tr = trace.cpu().numpy()
    assert np.isfinite(tr).all() and tr[-1] > tr[0]
    held = slice(8, 10)
    r = conversion.convert_gmm_diff_batch(model, S[held], ls[held], mc.CFG)
    d_lt, = evaluation._upload_lens(lt[held])
    cb = evaluation._cepstra_launch(evaluation._mel_launch(torch.from_numpy(T[held]).cuda(), d_lt, mc.CFG), 24, 1)
    scale = 1.0 / (4.0 * mc.CFG['M_dB_norm_factor'])
    frames_t = [1 + l // hop for l in lt[held]]
    before = float(evaluation.dtw_batch(r.cep_src, cb, r.n_frames, frames_t, scale=scale).mcd.mean())
    after = float(evaluation.dtw_batch(r.cep_pred, cb, r.n_frames, frames_t, scale=scale).mcd.mean())
    print('MEASURED realigned fit on 4 sentences: held-out MCD %.3f -> %.3f dB (converted cepstra)' % (before, after))
    assert after < before
    # 8 kHz in, 8 kHz out, denoised
    S8 = audio_lib.resample_batch(S[held], ls[held], 16000, 8000)
    w8, l8 = S8[0].cpu().numpy(), [int(v) for v in S8[1]]
    r8 = conversion.convert_gmm_diff_batch(model, w8, l8, mc.CFG, wav_sr=8000, out_sr=8000, denoise=True)
    l16 = hop * (audio_lib.resample_len(np.array(l8), 8000, 16000) // hop)
    assert r8.n_frames == [1 + int(l) // hop for l in l16]
    assert r8.n_samples == [int(v) for v in audio_lib.resample_len(hop * (np.array(r8.n_frames) - 1), 16000, 8000)]
    y = r8.y_wav_pred.cpu().numpy()
    assert np.isfinite(y).all() and all(np.abs(y[b, :n]).max() > 0 and not y[b, n:].any() for b, n in enumerate(r8.n_samples))
