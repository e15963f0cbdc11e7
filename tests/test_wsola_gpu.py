"""Waveform time scaling on the device (csrc/vc_wsola.hip): vc_wsola_plan and vc_wsola_ola_f32 bit for bit against the numpy
restatement of tests/wsola_ref.py, the identity map and the periodic-extension property on the device, graph replay, and
conversion.convert_diff_duration_batch on the decoder that the convert_batch tests build.

The plan kernel deals candidate PAIRS (2 p, 2 p + 1; the last pair holds one candidate) to 512 lanes.  Up to 256 pairs,
G = min(512 / pairs, 8) lanes share a pair's window; beyond, lane t takes pairs t, t + 512, ...  With tol + 1 pairs the seams
of that mapping lie between tol 63 | 64 (G 8 | 7), 72 | 73 (7 | 6), 84 | 85 (6 | 5), 101 | 102 (5 | 4), 127 | 128 (4 | 3),
169 | 170 (3 | 2), 255 | 256 (2 | 1), 511 | 512 (one round | two) and 1023 | 1024 (two | three): SEAM_TOLS, run at hop 80,
group 2.  A window's S dwords are cut at multiples of 4 and walked 8, 4 and 1 at a time: CONFIGS has S of 1, 2, 4, 8, 16, 32,
80, 160, 255, 320, 1020 and 1024."""
from collections import namedtuple

import numpy as np
import pytest
import torch

import wsola_ref as wr
from test_convert_batch_gpu import _ragged, f32_models      # noqa: F401  (f32_models: a module-scoped fixture)
from test_wsola_cpu import inner_map, periodic

pytestmark = pytest.mark.gpu

Q = wr.Q
POISON = 0x7FC00000                     # a NaN's bits: what an unwritten int32 output would still hold
Plans = namedtuple('plans', 'a cost n_grains out_len')
# (hop, group, tol): hop in {1, 8, 80, 255}, group in {1, 2, 4}, S = 1024 once, tol 0, 1, 1024 and both sides of every seam
CONFIGS = [(8, 2, 12), (1, 1, 0), (1, 4, 1), (80, 2, 160), (80, 1, 63), (255, 4, 64), (255, 1, 255), (8, 4, 511), (8, 2, 512),
           (80, 4, 510), (8, 1, 767), (1, 2, 768), (80, 2, 1023), (512, 2, 1024)]
SEAM_TOLS = (63, 64, 72, 73, 84, 85, 101, 102, 127, 128, 169, 170, 255, 256, 511, 512, 1024)
ALL_CONFIGS = CONFIGS + [(80, 2, t) for t in SEAM_TOLS]
MAX_LEN = 5000


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run_plan(x, lens, pos, n_out, hop, g, tol, qscale=32768.0, max_len=None):
    """vc_wsola_plan itself on outputs that hold NaN bits; checks that the inputs are what they were."""
    import _vc
    lib = _vc.lib()
    B, stride = x.shape
    F = pos.shape[1]
    max_len = stride if max_len is None else max_len
    M = lib.vc_wsola_max_grains(F, hop, g)
    assert M == wr.max_grains(F, hop, hop * g)
    ins = [np.asarray(x, np.float32), np.asarray(lens, np.int32), np.asarray(pos, np.int32), np.asarray(n_out, np.int32)]
    d = [_dev(a) for a in ins]
    n = torch.full((2, B), POISON, dtype=torch.int32, device='cuda')
    tab = torch.full((2, B, M), POISON, dtype=torch.int32, device='cuda')
    _vc.check(lib.vc_wsola_plan(_vc.ptr(d[0]), stride, _vc.ptr(d[1]), _vc.ptr(d[2]), _vc.ptr(d[3]), B, max_len, F, hop, g, tol, qscale,
                                _vc.ptr(tab[0]), _vc.ptr(tab[1]), _vc.ptr(n[0]), _vc.ptr(n[1]), _vc.current_stream()))
    torch.cuda.synchronize()
    for a, t in zip(ins, d):
        assert np.array_equal(t.cpu().numpy().view(np.int32), a.view(np.int32))
    n, tab = n.cpu().numpy(), tab.cpu().numpy()
    return Plans(tab[0], tab[1], n[0], n[1])


def ref_plans(x, lens, pos, n_out, hop, g, tol, qscale=32768.0, max_len=None):
    rows = [wr.plan(x[b], lens[b], pos[b], n_out[b], hop, g, tol, qscale, max_len=max_len) for b in range(len(lens))]
    return Plans(np.array([r.a for r in rows], np.int32), np.array([r.cost for r in rows], np.int32),
                 np.array([r.K for r in rows], np.int32), np.array([r.out_len for r in rows], np.int32))


def same_plans(got, want, what=''):
    for name, g, w in zip(Plans._fields, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError('%s %s: %d of %d differ, first at %s: device %s, reference %s'
                                 % (what, name, len(bad), g.size, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


KINDS = ('noise', 'clip', 'zero', 'const', 'periodic', 'specials', 'noise', 'voiced', 'noise')


def ragged_batch(hop, g, tol, seed):
    """Nine utterances of len 1, S - 1, S, S + 1, 2 S + 1, 1023, 1024, 1025 and 5000 in rows of 5,000 samples that hold NaN
    from len on; a signal kind and a map kind per row, dealt anew per configuration: maps that are monotone at a random rate,
    junk (any int32: negative, beyond the input, not monotone) or the identity; n_out of 0, 1, 2, out_frames or less."""
    rng = np.random.RandomState(seed)
    S = hop * g
    lens = np.array([1, S - 1, S, S + 1, 2 * S + 1, 1023, 1024, 1025, MAX_LEN], np.int32)
    B, F = len(lens), 2 + 6 * g
    x = np.full((B, MAX_LEN), np.nan, np.float32)
    kinds = rng.permutation(KINDS)
    for b, n in enumerate(lens):
        t = np.arange(n)
        v = {'noise': lambda: 0.3 * rng.standard_normal(n), 'clip': lambda: 3.0 * rng.standard_normal(n), 'zero': lambda: np.zeros(n),
             'const': lambda: np.full(n, 0.37), 'periodic': lambda: rng.uniform(-0.9, 0.9, 11)[t % 11],
             'specials': lambda: np.where(rng.rand(n) < 0.1, rng.choice([np.nan, np.inf, -np.inf, 1e30, -0.0], n), rng.standard_normal(n)),
             'voiced': lambda: 0.5 * np.sin(2 * np.pi * t / 91.7) + 0.2 * np.sin(2 * np.pi * t / 30.57 + 1.0)}[kinds[b]]()
        x[b, :n] = v
    pos = np.zeros((B, F), np.int32)
    maps = rng.permutation(['rate'] * 5 + ['junk'] * 2 + ['identity', 'rate'])
    for b, n in enumerate(lens):
        if maps[b] == 'junk':
            pos[b] = rng.randint(-2 ** 31, 2 ** 31, F).astype(np.int64).astype(np.int32)
            k = rng.rand(F) < 0.5
            pos[b, k] = rng.randint(0, (int(n) // hop + 3) << 16, int(k.sum()))
        elif maps[b] == 'identity':
            pos[b] = np.arange(F, dtype=np.int64) << 16
        else:
            pos[b] = np.rint(np.cumsum(rng.uniform(0.2, 2.5, F)) * (rng.uniform(0.0, 1.2) * (int(n) / hop / F) * Q)).clip(0, 2 ** 31 - 1)
    n_out = rng.permutation([F, F, F, F - 1, F, 2, F, 1, 0]).astype(np.int32)
    n_out[-1] = F                                                   # the longest utterance always runs the whole chain
    return x, lens, pos, n_out


_ragged_cache = {}


def ragged_run(cfg):
    if cfg not in _ragged_cache:
        hop, g, tol = cfg
        ins = ragged_batch(hop, g, tol, 1000 + ALL_CONFIGS.index(cfg))
        _ragged_cache[cfg] = (ins, ref_plans(*ins, hop, g, tol))
    return _ragged_cache[cfg]


@pytest.mark.parametrize('cfg', ALL_CONFIGS, ids=lambda c: 'hop%d-g%d-tol%d' % c)
def test_plan_bit_exact_on_a_ragged_batch(cfg):
    hop, g, tol = cfg
    ins, want = ragged_run(cfg)
    got = run_plan(*ins, hop, g, tol)
    same_plans(got, want, str(cfg))
    K = want.n_grains
    assert K[-1] == want.a.shape[1] and K[-1] >= 7 and (K == 0).sum() >= 1
    for b in range(len(K)):                                         # the padding, spelled out
        assert (got.a[b, K[b]:] == -2 ** 31).all() and (got.cost[b, K[b]:] == -1).all()


def test_plan_across_the_tiles_of_512_steps():
    """The kernel computes its targets and writes its results 512 steps at a time: chains of 1, 511, 512, 513, 1023, 1024,
    1025 and 1199 steps (hop 1, group 1: K = n_out)."""
    hop, g, tol, F = 1, 1, 2, 1200
    rng = np.random.RandomState(77)
    n_out = np.array([2, 512, 513, 514, 1024, 1025, 1026, F], np.int32)
    lens = np.full(len(n_out), 1300, np.int32)
    x = (0.3 * rng.standard_normal((len(n_out), 1300))).astype(np.float32)
    pos = np.stack([np.rint(np.cumsum(rng.uniform(0.2, 1.8, F)) * Q).astype(np.int64).astype(np.int32) for _ in n_out])
    want = ref_plans(x, lens, pos, n_out, hop, g, tol)
    same_plans(run_plan(x, lens, pos, n_out, hop, g, tol), want, 'tiles of steps')
    assert want.n_grains.tolist() == n_out.tolist() and len(set(want.a[-1, 1:F] - np.array(pos[-1, 1:F] >> 16))) > 1


def test_every_utterance_alone_under_other_sizes():
    """Each row of one ragged batch again as a batch of one, with another max_len (and row stride) and more output frames."""
    cfg = CONFIGS[0]
    hop, g, tol = cfg
    (x, lens, pos, n_out), want = ragged_run(cfg)
    for b in range(len(lens)):
        L1 = int(lens[b]) + 37
        x1 = np.full((1, L1), np.nan, np.float32)
        x1[0, :lens[b]] = x[b, :lens[b]]
        p1 = np.full((1, pos.shape[1] + 3), -1, np.int32)
        p1[0, :pos.shape[1]] = pos[b]
        one = run_plan(x1, lens[b:b + 1], p1, n_out[b:b + 1], hop, g, tol)
        M = want.a.shape[1]
        assert one.a.shape[1] >= M and np.array_equal(one.a[0, :M], want.a[b]) and np.array_equal(one.cost[0, :M], want.cost[b]), b
        assert one.n_grains[0] == want.n_grains[b] and one.out_len[0] == want.out_len[b]
        assert (one.a[0, M:] == -2 ** 31).all() and (one.cost[0, M:] == -1).all()


def test_lengths_and_counts_beyond_their_bounds_are_clamped_and_qscale_scales():
    hop, g, tol = 8, 2, 12
    rng = np.random.RandomState(3)
    x = (0.3 * rng.standard_normal((4, 600))).astype(np.float32)
    pos = np.stack([wr.identity_map(30)] * 4)
    lens = np.array([601, 2 ** 31 - 1, -5, 400], np.int32)
    n_out = np.array([31, -2 ** 31, 30, 2 ** 31 - 1], np.int32)
    for qscale, max_len in ((32768.0, 600), (100.0, 450), (3.0e38, 600), (1e-3, 600)):
        got = run_plan(x, lens, pos, n_out, hop, g, tol, qscale, max_len=max_len)
        same_plans(got, ref_plans(x, lens, pos, n_out, hop, g, tol, qscale, max_len=max_len), 'qscale %g' % qscale)
        assert got.n_grains.tolist() == [16, 0, 0, 16]


def test_limits_and_argument_checks():
    import _vc
    import conversion
    lib = _vc.lib()
    i, o = (torch.zeros(64, dtype=torch.int32, device='cuda') for _ in range(2))
    f, fo = (torch.zeros(64, dtype=torch.float32, device='cuda') for _ in range(2))
    p, q, pf, st = _vc.ptr(i), _vc.ptr(o), _vc.ptr(f), _vc.current_stream()
    plan = lambda B=1, L=16, F=2, hop=8, g=2, tol=4, qs=32768.0, x=pf, stride=None: lib.vc_wsola_plan(
        x, L if stride is None else stride, p, p, p, B, L, F, hop, g, tol, qs, q, q, q, q, st)
    ola = lambda B=1, L=16, F=2, hop=8, g=2, y=_vc.ptr(fo): lib.vc_wsola_ola_f32(pf, L, p, p, p, p, pf, B, L, F, hop, g, y, st)
    assert plan() == 0 and ola() == 0
    for kw in (dict(B=65536), dict(L=2 ** 24 + 1), dict(F=16385), dict(hop=1025, g=1), dict(hop=513, g=2), dict(g=1025, hop=1), dict(tol=1025)):
        assert plan(**kw) == 4, kw                                  # VC_ERR_UNSUPPORTED
        if 'tol' not in kw:
            assert ola(**kw) == 4, kw
    for kw in (dict(B=0), dict(L=0), dict(F=0), dict(hop=0), dict(g=0), dict(tol=-1), dict(qs=0.0), dict(qs=-1.0), dict(qs=float('inf')),
               dict(qs=float('nan')), dict(x=None), dict(stride=15)):
        assert plan(**kw) == 1, kw                                  # VC_ERR_INVALID
    assert ola(y=pf) == 1 and ola(y=None) == 1 and ola(B=0) == 1    # in place; no output
    assert ola(F=1, y=None) == 0                                    # a row of no samples: nothing to write
    assert lib.vc_wsola_max_grains(16384, 1024, 1) == 16384 and lib.vc_wsola_max_grains(16385, 8, 2) == 0
    assert lib.vc_wsola_max_grains(10, 513, 2) == 0 and lib.vc_wsola_max_grains(1, 8, 2) == 1 and lib.vc_wsola_max_grains(0, 8, 2) == 0
    torch.cuda.synchronize()
    wav, pos = np.zeros((2, 400), np.float32), np.zeros((2, 5), np.int32)
    for bad in (dict(hop_length=1025), dict(group=0), dict(tol=1025), dict(qscale=0.0), dict(lens=[401, 1]), dict(n_out=[6, 1]),
                dict(pos=pos[:1]), dict(wav=_dev(wav).double())):
        with pytest.raises(ValueError):
            conversion.time_scale_batch(**dict(dict(wav=wav, lens=[400, 300], pos=pos, n_out=[5, 2], hop_length=80), **bad))


# ------------------------------------------------------------------------------------------------ overlap-add
def run_ola(x, lens, a, n_grains, out_len, hop, g, F, max_len=None):
    """vc_wsola_ola_f32 itself on a plan given as numpy arrays, the output NaN first; the inputs must come back untouched."""
    import _vc
    import conversion
    B, stride = x.shape
    max_len = stride if max_len is None else max_len
    L = hop * (F - 1)
    ins = [np.asarray(x, np.float32), np.asarray(lens, np.int32), np.asarray(a, np.int32), np.asarray(n_grains, np.int32),
           np.asarray(out_len, np.int32)]
    d = [_dev(v) for v in ins]
    assert ins[2].shape == (B, wr.max_grains(F, hop, hop * g))
    y = torch.full((B, L), float('nan'), dtype=torch.float32, device='cuda')
    _vc.check(_vc.lib().vc_wsola_ola_f32(_vc.ptr(d[0]), stride, _vc.ptr(d[1]), _vc.ptr(d[2]), _vc.ptr(d[3]), _vc.ptr(d[4]),
                                         _vc.ptr(conversion.wsola_window(hop * g, 'cuda')), B, max_len, F, hop, g, _vc.ptr(y),
                                         _vc.current_stream()))
    torch.cuda.synchronize()
    for v, t in zip(ins, d):
        assert np.array_equal(t.cpu().numpy().view(np.int32), v.view(np.int32))
    return y.cpu().numpy()


def same_ola(got, x, lens, a, n_grains, out_len, hop, g, F, what, max_len=None):
    for b in range(len(lens)):
        want = wr.ola(x[b], lens[b], a[b], n_grains[b], out_len[b], hop * g, hop * (F - 1), max_len=max_len)
        if not np.array_equal(got[b].view(np.int32), want.view(np.int32)):
            bad = np.flatnonzero(got[b].view(np.int32) != want.view(np.int32))
            raise AssertionError('%s utterance %d: %d of %d samples differ, first at %d: device %r, reference %r'
                                 % (what, b, len(bad), len(want), bad[0], got[b, bad[0]], want[bad[0]]))


@pytest.mark.parametrize('cfg', [CONFIGS[0], CONFIGS[3], CONFIGS[5], CONFIGS[-1]], ids=lambda c: 'hop%d-g%d-tol%d' % c)
def test_ola_bit_exact_on_the_restatements_plans(cfg):
    hop, g, tol = cfg
    (x, lens, pos, n_out), want = ragged_run(cfg)
    x = np.where(np.isfinite(x), x, np.float32(0.25))              # (inf - inf: a NaN whose sign is the platform's)
    x[np.arange(MAX_LEN)[None, :] >= lens[:, None]] = np.nan        # beyond len: never read
    got = run_ola(x, lens, want.a, want.n_grains, want.out_len, hop, g, pos.shape[1])
    same_ola(got, x, lens, want.a, want.n_grains, want.out_len, hop, g, pos.shape[1], str(cfg))
    assert np.isfinite(got).all() and np.abs(got).max() > 0


@pytest.mark.parametrize('F', [1024, 1025, 1026])
def test_ola_either_side_of_the_tile(F):
    """hop 1: rows of 1023, 1024 and 1025 outputs (a tile holds 1,024), output lengths up to the row and just below."""
    hop, g, tol = 1, 16, 16
    rng = np.random.RandomState(F)
    n = 1400
    x = (0.3 * rng.standard_normal((3, n))).astype(np.float32)
    lens = np.array([n, 1200, 1030], np.int32)
    pos = np.stack([np.rint(np.arange(F) * r * Q).astype(np.int64).astype(np.int32) for r in (1.0, 1.1, 0.8)])
    n_out = np.array([F, F - 1, F - 2], np.int32)
    want = ref_plans(x, lens, pos, n_out, hop, g, tol)
    same_plans(run_plan(x, lens, pos, n_out, hop, g, tol), want, 'F %d' % F)
    got = run_ola(x, lens, want.a, want.n_grains, want.out_len, hop, g, F)
    same_ola(got, x, lens, want.a, want.n_grains, want.out_len, hop, g, F, 'F %d' % F)
    assert want.out_len.tolist() == [F - 1, F - 2, F - 3] and np.array_equal(got[0], x[0, :F - 1])


def test_ola_on_a_plan_made_by_hand():
    """Grains that reach before sample 0 and past len, a at both guards and one beyond, counts and lengths beyond their
    rows, a plan of junk: nothing but samples of [0, len) is read, everything else counts as 0."""
    hop, g, F = 8, 2, 21                                            # S = 16, rows of 160 outputs, M = 11 grains
    M, L = 11, 160
    rng = np.random.RandomState(8)
    n = 300
    x = np.full((6, 320), np.nan, np.float32)
    x[:, :n] = rng.standard_normal((6, n))
    lens = np.array([2 ** 31 - 1] + [n] * 5, np.int32)             # (the first clamps to max_len)
    a = np.zeros((6, M), np.int32)
    a[0] = [-20, -16, -5, 0, 3, n - 20, n - 16, n - 1, n, n + 40, 7]
    a[1] = [2 ** 24, -2 ** 24, 2 ** 24 + 1, -2 ** 24 - 1, 5, 2 ** 31 - 1, -2 ** 31, 9, 2 ** 24 - 1, -2 ** 24 + 1, 11]
    a[2] = rng.randint(-2 ** 31, 2 ** 31, M).astype(np.int64)
    a[3] = np.arange(M) * 16
    a[4] = np.arange(M) * 16
    a[5] = rng.randint(-40, n + 40, M)
    n_grains = np.array([M, M, M, 2 ** 31 - 1, -3, 6], np.int32)
    out_len = np.array([L, L, L, 2 ** 31 - 1, L, -2 ** 31], np.int32)
    for max_len in (n, n + 10):
        xx = x.copy()
        xx[0, n:max_len] = 0.5                                      # utterance 0's len clamps to max_len: those are samples
        got = run_ola(xx, lens, a, n_grains, out_len, hop, g, F, max_len=max_len)
        same_ola(got, xx, lens, a, n_grains, out_len, hop, g, F, 'by hand', max_len=max_len)
        assert np.isfinite(got).all()
        assert np.array_equal(got[3], xx[3, :L]) and not got[4].any() and not got[5].any() and got[0].any()


# ------------------------------------------------------------------------------------------------ the two launches together
def test_identity_map_returns_the_signal_bit_for_bit():
    import conversion
    rng = np.random.RandomState(21)
    hop, F = 80, 60
    lens = [hop * F + 400, hop * 40 + 333, hop * 59]                # the last: the input ends where the map ends
    x = np.zeros((3, max(lens)), np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = 0.3 * rng.standard_normal(n)
    pos = np.stack([wr.identity_map(nf, F) for nf in (F, 41, F)])
    r = conversion.time_scale_batch(x, lens, pos, [F, 41, F], hop)
    y, ns = r.y.cpu().numpy(), r.n_samples.tolist()
    assert ns == [hop * (F - 1), hop * 40, hop * (F - 1)] and r.plan.tol == 160 and r.plan.group == 2 and tuple(y.shape) == (3, hop * (F - 1))
    for b in range(3):
        assert np.array_equal(y[b, :ns[b]].view(np.int32), x[b, :ns[b]].view(np.int32)) and not y[b, ns[b]:].any(), b
        want = wr.plan(x[b], lens[b], pos[b], [F, 41, F][b], hop)
        assert np.array_equal(r.plan.a[b].cpu().numpy(), want.a) and np.array_equal(r.plan.cost[b].cpu().numpy(), want.cost)
    dev = conversion.time_scale_batch(_dev(x), _dev(np.array(lens, np.int32)), _dev(pos), _dev(np.array([F, 41, F], np.int32)), hop)
    assert torch.equal(dev.y, r.y) and torch.equal(dev.plan.a, r.plan.a) and torch.equal(dev.n_samples, r.n_samples)


@pytest.mark.parametrize('P,tol,ok', [(7, 12, True), (25, 12, True), (26, 12, False), (13, 0, False)])
def test_periodic_extension_on_the_device(P, tol, ok):
    import conversion
    rng = np.random.RandomState(P + tol)
    rates = (0.5, 0.6, 1.37, 2.0, 0.9) if ok else ((16.0 / 29.0, 16.0 / 3.0) if P == 26 else (0.5, 0.6, 1.37, 2.0))
    maps = [inner_map(rng, 60, rate, jitter=0.6 if rate == 0.9 else 0.0) for rate in rates]
    n = max(m[1] for m in maps)
    x = np.stack([periodic(rng, P, n) for _ in maps])
    r = conversion.time_scale_batch(x, [m[1] for m in maps], np.stack([m[0] for m in maps]), [60] * len(maps), 8, group=2, tol=tol)
    y, a0 = r.y.cpu().numpy(), r.plan.a[:, 0].tolist()
    for b in range(len(maps)):
        want = x[b, (np.arange(8 * 59) + a0[b]) % P]
        bad = float(np.mean(y[b, 16:].view(np.int32) != want[16:].view(np.int32)))
        assert (bad == 0.0 and np.array_equal(y[b].view(np.int32), want.view(np.int32))) if ok else bad > 0.5, (b, bad)


def test_graph_replay_of_plan_and_ola():
    import conversion
    from test_graph_replay_gpu import _capture, _free, _same
    rng = np.random.RandomState(14)
    B, Lmax, hop, F = 3, 6000, 80, 90

    def inputs(k):
        lens = np.array([Lmax, Lmax - 977 * (k + 1), 170 + k], np.int32)
        n_out = np.array([F, F - 11 * k, 2 + k], np.int32)
        pos = np.stack([np.rint(np.cumsum(rng.uniform(0.3, 1.4, F)) * Q * lens[b] / hop / F).astype(np.int64).astype(np.int32) for b in range(B)])
        x = (0.3 * rng.standard_normal((B, Lmax))).astype(np.float32)
        return [_dev(x), _dev(lens), _dev(pos), _dev(n_out)]

    conversion.wsola_window(160, 'cuda')

    def chain(x, lens, pos, n_out):
        p = conversion._wsola_plan_launch(x, lens, pos, n_out, hop, 2, 160, 32768.0)
        return p.a, p.cost, p.n_grains, p.out_len, conversion._wsola_ola_launch(x, lens, p)

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
            for name, a, b in zip(('a', 'cost', 'n_grains', 'out_len', 'y'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert int(outs[2][0]) > 5 and float(outs[4][0].abs().max()) > 0
    finally:
        _free(g)


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def diff_run(f32_models):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_diff_batch(dec, wav, lens, c)
    torch.cuda.synchronize()
    return r


def test_convert_diff_duration_batch_is_the_separate_calls(f32_models, diff_run):
    import conversion
    import evaluation
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    hop, d = c['hop_length'], diff_run
    n_use = np.array(d.n_frames)
    # one rate for everything
    r = conversion.convert_diff_duration_batch(dec, wav, lens, c, rate=1.25)
    m = conversion.duration_map_batch(np.zeros((3, 1), np.int32), n_use[:, None].astype(np.int32), [1, 1, 1], n_use, ratio=1.25,
                                      max_frames=r.max_frames, min_frames=2)
    ts = conversion.time_scale_batch(d.y_wav_pred, d.n_samples, m.pos, m.n_out, hop)
    assert r.max_frames == int((n_use.max() * 81920 + 32768) >> 16) and r.max_samples == hop * (r.max_frames - 1) and r.src_frames == d.n_frames
    assert torch.equal(r.map.pos, m.pos) and torch.equal(r.n_frames, m.n_out) and r.flags.tolist() == [0, 0, 0]
    assert r.n_frames.tolist() == [int((n * 81920 + 32768) >> 16) for n in n_use] and r.n_samples.tolist() == [hop * (n - 1) for n in r.n_frames.tolist()]
    assert torch.equal(r.plan.a, ts.plan.a) and torch.equal(r.plan.cost, ts.plan.cost) and torch.equal(r.n_samples, ts.n_samples)
    assert torch.equal(r.y_wav_pred, ts.y) and tuple(r.y_wav_pred.shape) == (3, r.max_samples)
    for name in ('mel_true', 'mel_pred', 'stft_true', 'stft_pred', 'phn_pred', 'gain'):          # at the source's timing
        assert torch.equal(getattr(r, name), getattr(d, name)), name
    out = r.y_wav_pred.cpu().numpy()
    for b, n in enumerate(r.n_samples.tolist()):
        assert np.isfinite(out[b]).all() and not out[b, n:].any() and out[b, :n].any()
        assert (r.plan.a[b, :int(r.plan.n_grains[b])] >= -160).all() and int(r.plan.cost[b, 1:int(r.plan.n_grains[b])].max()) > 0
    # a rate per decoded phoneme class
    ratio = np.random.RandomState(9).choice([0.5, 0.8, 1.25, 2.0], 61).astype(np.float32)
    r2 = conversion.convert_diff_duration_batch(dec, wav, lens, c, ratio=ratio, gap_ratio=0.75, decode=dict(min_dur=2))
    dd = evaluation.decode_batch(d.phn_pred, d.n_frames, min_dur=2)
    m2 = conversion.duration_map_batch(dd.seg.start, dd.seg.end, dd.seg.n_seg, n_use, labels=dd.seg.labels, ratio=ratio, gap_ratio=0.75,
                                       max_frames=r2.max_frames, min_frames=2)
    ts2 = conversion.time_scale_batch(d.y_wav_pred, d.n_samples, m2.pos, m2.n_out, hop)
    assert torch.equal(r2.map.pos, m2.pos) and torch.equal(r2.n_frames, m2.n_out) and r2.flags.tolist() == [0, 0, 0]
    assert torch.equal(r2.seg.start, m2.out_start) and torch.equal(r2.seg.end, m2.out_end) and torch.equal(r2.seg.labels, dd.seg.labels)
    assert torch.equal(r2.y_wav_pred, ts2.y) and torch.equal(r2.plan.a, ts2.plan.a) and r2.n_frames.tolist() != d.n_frames
    assert torch.isfinite(r2.y_wav_pred).all()


def test_rate_one_is_convert_diff_batch(f32_models, diff_run):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_diff_duration_batch(dec, wav, lens, c, rate=1.0)
    assert r.n_frames.tolist() == diff_run.n_frames and r.n_samples.tolist() == diff_run.n_samples and r.max_frames == max(diff_run.n_frames)
    for b, n in enumerate(diff_run.n_samples):
        assert torch.equal(r.y_wav_pred[b, :n], diff_run.y_wav_pred[b, :n]) and not r.y_wav_pred[b, n:].any(), b
        K = int(r.plan.n_grains[b])
        assert r.plan.a[b, :K].tolist() == [160 * k for k in range(K)] and not r.plan.cost[b, :K].any()


def test_convert_diff_duration_batch_no_host_synchronisation_and_argument_checks(f32_models):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    d_wav = _dev(wav)
    ratio = _dev(np.linspace(0.6, 1.4, 61).astype(np.float32))
    calls = (dict(rate=1.5), dict(rate=0.75, pitch=1.2, out_sr=22050), dict(ratio=ratio, max_frames=2400, gap_ratio=1.2, group=1, tol=100))
    for kw in calls:                                                # warm-up
        conversion.convert_diff_duration_batch(dec, d_wav, lens, c, window_batch=4, **kw)
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        rs = [conversion.convert_diff_duration_batch(dec, d_wav, lens, c, window_batch=4, **kw) for kw in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.y_wav_pred).all() and float(r.y_wav_pred.abs().max()) > 0 for r in rs) and rs[2].flags.tolist() == [0, 0, 0]
    n1 = rs[1].n_frames.tolist()
    assert rs[1].n_samples.tolist() == [-(-80 * (n - 1) * 441 // 320) for n in n1] and rs[1].max_samples == -(-80 * (max(n1) - 1) * 441 // 320)
    assert rs[1].f0_src is not None and rs[0].f0_src is None and rs[2].plan.tol == 100 and rs[2].plan.group == 1
    for kw, msg in ((dict(rate=0.0), 'rate'), (dict(rate=8.5), 'rate'), (dict(rate=True), 'rate'), (dict(), 'exactly one'),
                    (dict(rate=1.0, ratio=[1.0] * 61), 'exactly one'), (dict(ratio=[1.0] * 61, out_len=np.zeros((3, 1200), np.int32)), 'exactly one'),
                    (dict(rate=0.001), 'frames'), (dict(ratio=ratio), 'max_frames'), (dict(rate=1.0, decode=dict(min_dur=2)), 'decode'),
                    (dict(ratio=[1.0] * 61, segments='argmax'), 'segments'), (dict(rate=1.0, group=13), 'group'), (dict(rate=1.0, tol=1025), 'tol'),
                    (dict(rate=1.0, qscale=0.0), 'qscale'), (dict(rate=1.0, pitch=2.5), 'pitch'), (dict(rate=1.0, alpha=2.0), 'alpha')):
        with pytest.raises(ValueError, match=msg):
            conversion.convert_diff_duration_batch(dec, d_wav, lens, c, **kw)
