"""Pitch conversion on the device (csrc/vc_pitch.hip): vc_psola_plan and vc_psola_ola_f32 bit for bit against the numpy
restatement of tests/pitch_ref.py, the identity within a derived rounding bound, a shifted vowel through the device's own
tracker, graph replay, and conversion.convert_pitch_batch on the decoder that the convert_batch tests build."""
from collections import namedtuple

import numpy as np
import pytest
import torch

import f0_ref
import pitch_ref as pr
from test_convert_batch_gpu import N_ITER, _ragged, f32_models      # noqa: F401  (f32_models: a module-scoped fixture)
from test_pitch_cpu import random_tables

pytestmark = pytest.mark.gpu

Q = pr.Q
POISON = 0x7FC00000                     # a NaN's bits: what an unwritten int32 output would still hold
LENS = (1, 15, 16, 17, 79, 80, 81, 1023, 1024, 1025, 4097, 20000)
Plans = namedtuple('plans', 'K J a s src h')


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run_plan(per, rat, lens, hop, Lmax):
    """vc_psola_plan itself on outputs that hold NaN bits; checks that the inputs are what they were."""
    import _vc
    lib = _vc.lib()
    B, F = per.shape
    M = lib.vc_psola_max_marks(Lmax)
    assert M == Lmax // 16 + 1
    ins = [np.asarray(a, np.int32) for a in (per, rat, lens)]
    d = [_dev(a) for a in ins]
    n = torch.full((2, B), POISON, dtype=torch.int32, device='cuda')
    tab = torch.full((4, B, M), POISON, dtype=torch.int32, device='cuda')
    _vc.check(lib.vc_psola_plan(_vc.ptr(d[0]), _vc.ptr(d[1]), _vc.ptr(d[2]), B, Lmax, F, hop, _vc.ptr(n[0]), _vc.ptr(n[1]),
                                _vc.ptr(tab[0]), _vc.ptr(tab[1]), _vc.ptr(tab[2]), _vc.ptr(tab[3]), _vc.current_stream()))
    torch.cuda.synchronize()
    for a, t in zip(ins, d):
        assert np.array_equal(t.cpu().numpy(), a)
    n, tab = n.cpu().numpy(), tab.cpu().numpy()
    return Plans(n[0], n[1], tab[0], tab[1], tab[2], tab[3])


def ref_plans(per, rat, lens, hop, Lmax):
    rows = [pr.plan(per[b], rat[b], lens[b], hop, pr.max_marks(Lmax)) for b in range(len(lens))]
    return Plans(*(np.array([getattr(r, f) for r in rows], np.int32) for f in Plans._fields))


def same_plans(got, want, what=''):
    for name, g, w in zip(Plans._fields, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError('%s %s: %d of %d differ, first at %s: device %s, reference %s'
                                 % (what, name, len(bad), g.size, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


EDGE = np.array([0, -1, -2 ** 31, 2 ** 31 - 1, 16 * Q, 16 * Q - 1, 1024 * Q, 1024 * Q + 1, Q // 2, Q // 2 - 1, 2 * Q, 2 * Q + 1, Q], np.int64)


def tables_of(kind, rng, B, hop, Lmax):
    n_fr = Lmax // hop
    F = dict(F1=1, F_short=max(1, n_fr // 3), F_long=2 * n_fr + 7).get(kind, 1 + n_fr)
    if kind == 'clamps':
        return rng.choice(EDGE, (B, F)).astype(np.int32), rng.choice(EDGE, (B, F)).astype(np.int32)
    if kind == 'alternating':                                       # voiced and unvoiced (period = hop) every other frame
        per = np.where(np.arange(F)[None, :] % 2 == 0, (rng.uniform(40, 270, (B, F)) * Q).astype(np.int64), hop << 16)
        return per.astype(np.int32), (2.0 ** rng.uniform(-1, 1, (B, F)) * Q).astype(np.int32)
    if kind == 'tie':                                               # ratio 2 on an even period: every other synthesis mark half way
        return np.full((B, F), 100 * Q, np.int32), np.full((B, F), 2 * Q, np.int32)
    t = [random_tables(rng, F) for _ in range(B)]
    return np.stack([p for p, _ in t]), np.stack([r for _, r in t])


@pytest.mark.parametrize('hop', [80, 1, 255])
@pytest.mark.parametrize('kind', ['random', 'clamps', 'F1', 'F_short', 'F_long', 'alternating', 'tie'])
def test_plan_bit_exact_on_a_ragged_batch(kind, hop):
    rng = np.random.RandomState(LENS.index(80) + hop)
    lens, Lmax = np.array(LENS, np.int32), max(LENS)
    per, rat = tables_of(kind, rng, len(lens), hop, Lmax)
    got = run_plan(per, rat, lens, hop, Lmax)
    want = ref_plans(per, rat, lens, hop, Lmax)
    same_plans(got, want, '%s hop %d' % (kind, hop))
    assert want.K[-1] >= 20 and (want.K >= 1).all() and (want.J >= 1).all()
    if kind == 'tie':
        b = len(lens) - 1
        s, src = want.s[b, :want.J[b]], want.src[b, :want.J[b]]
        assert ((s - src) == 50).sum() > 50 and not ((src - s) == 50).any()          # half way: the lower mark, never the upper
    if kind == 'random':                                            # each utterance alone, under another B, Lmax (and M)
        for b in range(len(lens)):
            L1 = int(lens[b]) + 37
            one = run_plan(per[b:b + 1], rat[b:b + 1], lens[b:b + 1], hop, L1)
            M1 = pr.max_marks(L1)
            m = min(M1, got.a.shape[1])
            for f in ('a', 's', 'src', 'h'):
                assert np.array_equal(getattr(one, f)[0, :m], getattr(got, f)[b, :m]), (b, f)
            assert one.K[0] == got.K[b] and one.J[0] == got.J[b] and (one.h[0, m:] == -1).all()


def test_plan_and_ola_limits_and_argument_checks():
    import _vc
    import conversion
    lib = _vc.lib()
    one = torch.zeros(64, dtype=torch.int32, device='cuda')
    f = torch.zeros(64, dtype=torch.float32, device='cuda')
    p = _vc.ptr(one)
    for B, L, F, hop in ((65536, 16, 1, 1), (1, 2 ** 24 + 1, 1, 1), (1, 16, 2 ** 20 + 1, 1), (1, 16, 1, 65537)):
        assert lib.vc_psola_plan(p, p, p, B, L, F, hop, p, p, p, p, p, p, _vc.current_stream()) == 4      # VC_ERR_UNSUPPORTED
    assert lib.vc_psola_plan(p, p, p, 1, 16, 1, 0, p, p, p, p, p, p, _vc.current_stream()) == 1
    assert lib.vc_psola_plan(p, None, p, 1, 16, 1, 1, p, p, p, p, p, p, _vc.current_stream()) == 1
    assert lib.vc_psola_ola_f32(_vc.ptr(f), p, p, p, p, p, _vc.ptr(f), 1, 2 ** 24 + 1, 0.5, _vc.ptr(one), _vc.current_stream()) == 4
    assert lib.vc_psola_ola_f32(_vc.ptr(f), p, p, p, p, p, _vc.ptr(f), 1, 16, 0.0, _vc.ptr(one), _vc.current_stream()) == 1
    assert lib.vc_psola_ola_f32(_vc.ptr(f), p, p, p, p, p, _vc.ptr(f), 1, 16, 0.5, _vc.ptr(f), _vc.current_stream()) == 1      # in place
    assert lib.vc_psola_max_marks(2 ** 24) == 2 ** 20 + 1 and lib.vc_psola_max_marks(2 ** 24 + 1) == 0 and lib.vc_psola_max_marks(0) == 0
    tab = np.full((2, 5), 100 * Q, np.int32)
    wav, f0 = np.zeros((2, 400), np.float32), np.full((2, 5), 160.0, np.float32)
    for bad in (lambda: conversion.psola_plan_batch(tab, tab[:1], [400, 400], 80), lambda: conversion.psola_plan_batch(tab, tab, [400, 401], 80, max_len=400),
                lambda: conversion.psola_plan_batch(tab, tab, [400, 400], 0), lambda: conversion.psola_plan_batch(tab, tab, [400, 400], 65537),
                lambda: conversion.psola_plan_batch(tab, tab, _dev(np.array([400, 400], np.int32)), 80),
                lambda: conversion.psola_plan_batch(tab, tab, [400, 400], 80, max_len=2 ** 24 + 1),
                lambda: conversion.pitch_shift_batch(wav, [400, 400], f0, 16000, 80), lambda: conversion.pitch_shift_batch(wav, [400, 400], f0, 16000, 80, ratio=2.5),
                lambda: conversion.pitch_shift_batch(wav, [400, 400], f0, 16000, 80, ratio=1.0, target_f0=f0),
                lambda: conversion.pitch_shift_batch(wav, [400, 401], f0, 16000, 80, ratio=1.0), lambda: conversion.pitch_shift_batch(wav, [400, 400], f0[:1], 16000, 80, ratio=1.0),
                lambda: conversion.pitch_shift_batch(wav, [400, 400], f0, 16000, 80, ratio=1.0, w_floor=0.0),
                lambda: conversion.pitch_shift_batch(wav.astype(np.float64)[0], [400], f0, 16000, 80, ratio=1.0)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ overlap-add
def run_ola(x, lens, plans, w_floor=0.5):
    """vc_psola_ola_f32 itself on plans given as numpy arrays, the output NaN first; the inputs must come back untouched."""
    import _vc
    import conversion
    B, Lmax = x.shape
    d_x, d_len = _dev(x), _dev(np.asarray(lens, np.int32))
    d = [_dev(np.asarray(getattr(plans, f), np.int32)) for f in ('J', 's', 'src', 'h')]
    assert d[1].shape == (B, pr.max_marks(Lmax))
    y = torch.full((B, Lmax), float('nan'), dtype=torch.float32, device='cuda')
    _vc.check(_vc.lib().vc_psola_ola_f32(_vc.ptr(d_x), _vc.ptr(d_len), _vc.ptr(d[0]), _vc.ptr(d[1]), _vc.ptr(d[2]), _vc.ptr(d[3]),
                                         _vc.ptr(conversion.psola_window('cuda')), B, Lmax, float(w_floor), _vc.ptr(y), _vc.current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint32), x.view(np.uint32))
    for t, f in zip(d, ('J', 's', 'src', 'h')):
        assert np.array_equal(t.cpu().numpy(), np.asarray(getattr(plans, f), np.int32))
    return y.cpu().numpy()


def hand_plan(M, s, src, h):
    pad = lambda v: np.array(list(v) + [-1] * (M - len(v)), np.int32)
    return pr.Plan(0, len(s), pad([]), pad(s), pad(src), pad(h))


@pytest.fixture(scope='module')
def ola_batch():
    """One ragged batch that holds every case of the overlap-add: per utterance (len, tables or a hand-made plan)."""
    rng = np.random.RandomState(11)
    hop, Lmax = 80, 5200
    M, F = pr.max_marks(Lmax), 1 + Lmax // hop
    const = lambda p, r: (np.full(F, int(p * Q), np.int32), np.full(F, int(r * Q), np.int32))
    alt = np.where(np.arange(F) % 2 == 0, (rng.uniform(40, 270, F) * Q).astype(np.int64), hop << 16).astype(np.int32)
    rows = [(5000, const(16, 1.0)),                                 # h of 16: up to 192 grains reach a tile
            (5200, const(1024, 1.0)),                               # h of 1024: grains that begin before a tile and end after it
            (5000, const(300.5, 2.0)),                              # more than two covering grains
            (4097, const(64, 0.5)),                                 # synthesis step 128, h 64: the samples half way are covered by no grain
            (3000, const(1024, 2.0)), (2049, const(1024, 0.5)),
            (5111, (alt, (2.0 ** rng.uniform(-1, 1, F) * Q).astype(np.int32))),
            (1, const(100, 1.0)), (1023, const(100, 1.3)), (1024, const(100, 0.7)), (1025, const(100, 1.0)), (2048, const(77, 1.9)),
            (5200, random_tables(rng, F)),
            # hand-made: a grain that starts before tile 1 and one that ends after it, sources that leave [0, len) on both sides
            (4500, hand_plan(M, [1000, 2100, 4000, 4490], [500, 2100, 4400, 3], [1024, 1024, 200, 16]))]
    lens = np.array([r[0] for r in rows], np.int32)
    plans = [r[1] if isinstance(r[1], pr.Plan) else pr.plan(r[1][0], r[1][1], r[0], hop, M) for r in rows]
    x = rng.standard_normal((len(rows), Lmax)).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, n:] = np.nan                                           # never read: a NaN would reach every output it touches
    return dict(x=x, lens=lens, plans=plans, stacked=Plans(*(np.array([getattr(p, f) for p in plans], np.int32) for f in Plans._fields)))


@pytest.mark.parametrize('w_floor', [0.5, 0.03])
def test_ola_bit_exact_on_plans_from_the_restatement(ola_batch, w_floor):
    """The division is IEEE (the compiler's v_div_scale / v_rcp / v_fma / v_div_fmas / v_div_fixup sequence under the
    project's flags), so y itself is compared bit for bit."""
    b = ola_batch
    got = run_ola(b['x'], b['lens'], b['stacked'], w_floor)
    assert not np.isnan(got).any()
    for i, (n, p) in enumerate(zip(b['lens'], b['plans'])):
        want, D = pr.ola(b['x'][i], n, p, w_floor)
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (i, int((got[i] != want).sum()), np.abs(got[i] - want).max())
        assert not got[i, n:].any()
        G = pr.coverage(len(want), n, p)
        assert not got[i][(G == 0)].any()                           # no grain: an exact zero
    G = [pr.coverage(5200, n, p)[:n] for n, p in zip(b['lens'], b['plans'])]
    assert G[0].max() >= 2 and G[2].max() >= 4 and (G[3] == 0).sum() >= 25 and G[1].min() >= 1
    outside = lambda p, n: any((int(p.src[j]) - int(p.h[j]) + 1 < 0) or (int(p.src[j]) + int(p.h[j]) - 1 >= n) for j in range(p.J))
    assert outside(b['plans'][2], 5000) and outside(b['plans'][-1], 4500)


def test_ola_reads_a_broken_plan_defensively():
    """A plan of junk (counts, marks, sources and widths of any value) forms no address: the launch returns finite values
    and zeros from len on."""
    rng = np.random.RandomState(12)
    Lmax, M = 3000, pr.max_marks(3000)
    junk = lambda shape: rng.choice(np.array([0, -1, 5, 1500, 2999, 3000, 10 ** 6, 2 ** 31 - 1, -2 ** 31], np.int64), shape).astype(np.int32)
    plans = Plans(junk(3), np.array([M, 2 ** 31 - 1, -7], np.int32), junk((3, M)), junk((3, M)), junk((3, M)), junk((3, M)))
    x = rng.standard_normal((3, Lmax)).astype(np.float32)
    got = run_ola(x, [3000, 1700, 2000], plans)
    assert np.isfinite(got).all() and not got[1, 1700:].any() and not got[2].any()


def test_identity_on_the_device():
    """Ratio 1 on a random contour through the public path.  The bound, per sample n with G grains covering it (src = s, so
    every grain contributes x[n] * w_g): N is G rounded products and G - 1 rounded sums of terms of one sign, relative
    error at most G u (u = 2^-24); D is G - 1 rounded sums of positive terms, at most (G - 1) u; the quotient adds u.  Where
    D >= w_floor the divisor is D itself, so |y - x| <= (2 G u + O(u^2)) |x|; c = 2 G + 1 covers the second-order terms.
    (x is normal noise and w >= W[2047] > 5e-7: no product underflows.)"""
    import conversion
    rng = np.random.RandomState(13)
    hop, lens = 80, [6070, 4001]
    F = 1 + max(lens) // hop
    f0 = (150.0 * 2.0 ** (0.5 * np.sin(np.arange(F) / 7.0 + np.array([[0.0], [1.0]])))).astype(np.float32)
    f0[:, 30:34] = 0.0
    x = rng.standard_normal((2, max(lens))).astype(np.float32)
    r = conversion.pitch_shift_batch(x, lens, f0, 16000, hop, ratio=1.0)
    y = r.y.cpu().numpy()
    per, rat = pr.tables(f0, 16000, ratio=1.0, unvoiced_period=hop)
    assert np.array_equal(r.period_q.cpu().numpy(), per) and np.array_equal(r.ratio_q.cpu().numpy(), rat)
    for b, n in enumerate(lens):
        _, D, p = pr.shift(x[b], n, per[b], rat[b], hop)
        assert np.array_equal(r.plan.s[b].cpu().numpy(), p.s) and int(r.plan.n_s[b]) == p.J
        live = D[:n] >= 0.5
        assert live.mean() > 0.9 and not live.all()        # (a jump of the period leaves samples under the floor: not scored)
        G = pr.coverage(len(x[b]), n, p)[:n]
        bound = (2 * G + 1) * 2.0 ** -24 * np.abs(x[b, :n]).astype(np.float64)
        err = np.abs(y[b, :n].astype(np.float64) - x[b, :n])
        print('identity: utterance %d, worst error / bound %.3f, G up to %d' % (b, (err[live] / bound[live]).max(), G[live].max()))
        assert (err[live] <= bound[live]).all() and not y[b, n:].any()


def test_a_shifted_vowel_through_the_devices_tracker():
    import conversion
    import evaluation
    n = [8000, 7000]
    x = np.zeros((2, 8000), np.float32)
    for b, hz in enumerate((210.0, 90.0)):
        x[b, :n[b]] = pr.vowel(np.full(n[b], hz))
    f = evaluation.f0_track_batch(x, n)
    d_n = _dev(np.array(n, np.int32))
    r = conversion.pitch_shift_batch(_dev(x), d_n, f.f0, 16000, 80, ratio=1.25)                # lengths that live on the device
    host = conversion.pitch_shift_batch(x, n, f.f0.cpu().numpy(), 16000, 80, ratio=1.25)
    assert torch.equal(r.y, host.y)
    g = evaluation.f0_track_batch(r.y, n).f0.cpu().numpy()
    for b, hz in enumerate((210.0, 90.0)):
        keep = f0_ref.fully_voiced_frames(np.ones(n[b], bool), 80, 512, f0_ref.lag_range(16000)[1]) & (g[b, :1 + n[b] // 80] > 0)
        c = float(f0_ref.cents(np.median(g[b, :1 + n[b] // 80][keep]), hz * 1.25))
        print('%.0f Hz x 1.25 on the device: %.2f cents over %d frames' % (hz, c, keep.sum()))
        assert keep.sum() >= 60 and abs(c) <= 20.0


def test_graph_replay_of_plan_and_ola():
    import conversion
    from test_graph_replay_gpu import _capture, _free, _same
    rng = np.random.RandomState(14)
    B, Lmax, hop = 3, 6000, 80
    F = 1 + Lmax // hop

    def inputs(k):
        lens = np.array([Lmax, Lmax - 977 * (k + 1), 17 + k], np.int32)
        t = [random_tables(rng, F) for _ in range(B)]
        return [_dev(np.stack([p for p, _ in t])), _dev(np.stack([r for _, r in t])), _dev(lens), _dev(rng.standard_normal((B, Lmax)).astype(np.float32))]

    def chain(per, rat, lens, x):
        p = conversion.psola_plan_batch(per, rat, lens, hop, max_len=Lmax)
        return p.n_a, p.n_s, p.a, p.s, p.src, p.h, conversion._psola_ola_launch(x, lens, p, 0.5)

    static = inputs(0)
    g, outs = _capture(lambda: chain(*static))
    try:
        for k in range(1, 3):
            new = inputs(k)
            for s, t in zip(static, new):
                s.copy_(t)
            g.replay()
            torch.cuda.synchronize()
            want = chain(*new)
            for name, a, b in zip(('n_a', 'n_s', 'a', 's', 'src', 'h', 'y'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert int(outs[1][0]) > 5 and float(outs[6][0].abs().max()) > 0
    finally:
        _free(g)


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def plain_run(f32_models):
    import conversion
    import evaluation
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_batch(dec, wav, lens, c, n_iter=N_ITER, phase='device', seed=5)
    f = evaluation.f0_track_batch(r.y_wav_pred, r.n_samples, sr=c['sample_rate'], hop_length=c['hop_length'])
    torch.cuda.synchronize()
    return r, f


def test_convert_pitch_batch_is_the_separate_calls(f32_models, plain_run):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    plain, f = plain_run
    wav, lens = _ragged()
    sr, hop = c['sample_rate'], c['hop_length']
    r = conversion.convert_pitch_batch(dec, wav, lens, c, pitch=1.25, n_iter=N_ITER, seed=5)
    sh = conversion.pitch_shift_batch(plain.y_wav_pred, plain.n_samples, f.f0, sr, hop, ratio=1.25)
    assert r.n_frames == plain.n_frames and r.n_samples == plain.n_samples and r.f0_target is None and r.y_wav_true is None
    for name in ('mel_true', 'mel_pred', 'stft_true', 'stft_pred', 'phn_pred'):
        assert torch.equal(getattr(r, name), getattr(plain, name)), name
    assert torch.equal(r.f0_pred, f.f0) and torch.equal(r.plan.s, sh.plan.s) and torch.equal(r.plan.src, sh.plan.src)
    assert torch.equal(r.y_wav_pred, sh.y) and not torch.equal(r.y_wav_pred, plain.y_wav_pred)
    assert all(not r.y_wav_pred[b, n:].any() for b, n in enumerate(plain.n_samples)) and torch.isfinite(r.y_wav_pred).all()
    # a contour to reach, per output frame
    target = (f.f0 * 1.1).cpu().numpy()
    r2 = conversion.convert_pitch_batch(dec, wav, lens, c, pitch=target, n_iter=N_ITER, seed=5)
    sh2 = conversion.pitch_shift_batch(plain.y_wav_pred, plain.n_samples, f.f0, sr, hop, target_f0=target)
    assert torch.equal(r2.y_wav_pred, sh2.y) and torch.equal(r2.f0_target.cpu(), torch.from_numpy(target))
    # ratio 1 changes no mark: the plan copies the analysis marks
    r1 = conversion.convert_pitch_batch(dec, wav, lens, c, pitch=1.0, n_iter=N_ITER, seed=5)
    assert torch.equal(r1.plan.s, r1.plan.a) and torch.equal(r1.plan.src, r1.plan.s) and torch.equal(r1.f0_pred, f.f0)


def test_convert_pitch_batch_no_host_synchronisation_and_argument_checks(f32_models, plain_run):
    import conversion
    import evaluation
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    plain, f = plain_run
    wav, lens = _ragged()
    d_wav = _dev(wav)
    f_in = evaluation.f0_track_batch(wav, lens)
    st_src = conversion.f0_stats_batch(f_in.f0, _dev(np.array(f_in.n_frames, np.int32)))
    st_tgt = conversion._F0_STATS_NT(st_src.count, st_src.mean + 0.2, st_src.std * 1.1)
    calls = (dict(pitch=0.8), dict(pitch=(f.f0 * 0.9)), dict(pitch='source'),
             dict(pitch='source', stats_src=st_src, stats_tgt=st_tgt, phase='spsi', out_sr=22050))
    for kw in calls:                                                # warm-up
        conversion.convert_pitch_batch(dec, d_wav, lens, c, n_iter=N_ITER, window_batch=4, **kw)
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        rs = [conversion.convert_pitch_batch(dec, d_wav, lens, c, n_iter=N_ITER, window_batch=4, **kw) for kw in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.y_wav_pred).all() for r in rs)
    # 'source': the input's own track, output frame u = input frame n_s + u (t_s = 0: n_s = 0)
    for b, n in enumerate(plain.n_frames):
        m = min(n, f_in.n_frames[b])
        assert torch.equal(rs[2].f0_target[b, :m], f_in.f0[b, :m]) and not rs[2].f0_target[b, m:].any()
    want = conversion.f0_transform(rs[2].f0_target, st_src, st_tgt)
    assert torch.equal(rs[3].f0_target, want)
    assert rs[3].n_samples == [-(-n * 441 // 320) for n in plain.n_samples]
    Fout = plain.mel_pred.shape[1]
    for kw, msg in ((dict(), 'pitch'), (dict(pitch=2.5), 'pitch'), (dict(pitch=0.3), 'pitch'), (dict(pitch=float('nan')), 'pitch'),
                    (dict(pitch=True), 'pitch'), (dict(pitch='target'), 'pitch'), (dict(pitch=np.ones((3, Fout - 1), np.float32)), 'contour'),
                    (dict(pitch=1.0, stats_src=st_src, stats_tgt=st_tgt), 'stats'), (dict(pitch='source', stats_src=st_src), 'stats'),
                    (dict(pitch=1.0, phase='numpy'), 'phase'), (dict(pitch=1.0, w_floor=0.0), 'w_floor'),
                    (dict(pitch=1.0, f0_args=dict(hop_length=40)), 'f0_args'), (dict(pitch=1.0, f0_args=dict(fmin=5.0)), 'fmin')):
        with pytest.raises(ValueError, match=msg):
            conversion.convert_pitch_batch(dec, d_wav, lens, c, n_iter=N_ITER, **kw)
