"""Forced alignment on the device (vc_align_f32 behind evaluation.align_batch) against the float32 restatement of
tests/align_ref.py: every output bit for bit.  The one exception the header names: a NaN is a NaN (sign and payload of a
NaN result are not compared)."""
import numpy as np
import pytest
import torch

import align_ref as ar
from test_convert_batch_gpu import _ragged, f32_models        # noqa: F401  (a fixture and its inputs; that file is not edited)

pytestmark = pytest.mark.gpu

INT_FIELDS = ('frame_state', 'start', 'end', 'n_visited')
F32_FIELDS = ('seg_score', 'total')
FRAMES = (1, 2, 15, 16, 17, 33, 130)          # the seams of the 16-frame code word and of the prefetch depth (4)
KINDS = ('int', 'logsoftmax', 'peaked', 'neginf', 'nan')


def _np(t):
    return t.detach().cpu().numpy()


def _canon(x):
    """float32 bits with every NaN mapped to one pattern."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).copy()
    b[np.isnan(x)] = 0x7fc00000
    return b


def _assert_equal(got, want, what=''):
    for k in INT_FIELDS:
        assert np.array_equal(_np(getattr(got, k)), getattr(want, k)), (what, k)
    for k in F32_FIELDS:
        assert np.array_equal(_canon(_np(getattr(got, k))), _canon(getattr(want, k))), (what, k)


def _log_softmax(x):
    x = x.astype(np.float32)
    m = x.max(-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)


def _scores(kind, F, C, seq, rng):
    """One utterance's scores [F, C] of the given kind; ``seq`` steers the speech-like kind so that it can be aligned."""
    if kind == 'int':
        return rng.randint(-3, 1, size=(F, C)).astype(np.float32)
    x = _log_softmax(rng.standard_normal((F, C)) * 2.0)
    if kind == 'peaked':
        S = len(seq)
        if F >= S:                                                  # a random split of the frames over the states
            cuts = np.sort(rng.choice(np.arange(1, F), size=S - 1, replace=False)) if S > 1 else np.array([], int)
            lens = np.diff(np.concatenate([[0], cuts, [F]]))
            p = ar.synthetic_posteriors(np.clip(seq, 0, C - 1), lens, C, seed=int(rng.randint(1 << 30)))
        else:
            p = ar.synthetic_posteriors(rng.randint(0, C, size=F), np.ones(F, int), C, seed=int(rng.randint(1 << 30)))
        return np.log(np.maximum(p, np.float32(1e-10))).astype(np.float32)
    if kind == 'neginf':
        x[rng.rand(F, C) < 0.3] = -np.inf
        x[rng.rand(F) < 0.1] = -np.inf
    if kind == 'nan':
        x[rng.randint(F)] = np.nan
        x[rng.randint(F), rng.randint(C)] = np.nan
    return x


def _batch(S, C, opt_mode, seed):
    """Every F of FRAMES x every kind, plus one utterance of S + 7 frames per kind 'int' and 'peaked' (so that the long
    sequences have feasible cases too): (score, seq, opt, n_frames, n_seq)."""
    rng = np.random.RandomState(seed)
    cases = [(F, k) for F in FRAMES for k in KINDS] + [(S + 7, 'int'), (S + 7, 'peaked')]
    B, Fmax = len(cases), max(max(FRAMES), S + 7)
    score = rng.standard_normal((B, Fmax, C)).astype(np.float32)    # rows beyond n_frames are NOT neutral
    seq = rng.randint(0, C, size=(B, S)).astype(np.int32)
    opt = None
    if opt_mode == 'sparse':
        opt = (rng.rand(B, S) < 0.15).astype(np.uint8)
    elif opt_mode == 'dense':
        opt = (rng.rand(B, S) < 0.8).astype(np.uint8)
        opt[::3] = 1
    n_frames = np.array([F for F, _ in cases], np.int32)
    for b, (F, k) in enumerate(cases):
        score[b, :F] = _scores(k, F, C, seq[b], rng)
    return score, seq, opt, n_frames, np.full((B,), S, np.int32)


@pytest.mark.parametrize('C', [1, 61, 256])
@pytest.mark.parametrize('S', [1, 2, 63, 64, 65, 128, 129, 257, 1024])
def test_bit_exact_against_the_float32_reference(S, C):
    """F over the code-word and prefetch seams x S over the lane-ownership seams (every K instantiation) x five kinds of
    scores x opt NULL / sparse / dense x C: all seven outputs."""
    import evaluation as ev
    n_feasible = 0
    for opt_mode in ('none', 'sparse', 'dense'):
        score, seq, opt, nf, ns = _batch(S, C, opt_mode, seed=S * 7 + C)
        want = ar.align_batch_f32(score, seq, opt, nf, ns)
        got = ev.align_batch(score, nf, seq, ns, optional=opt, kind='log')
        _assert_equal(got, want, opt_mode)
        lab = np.where(want.frame_state >= 0, np.take_along_axis(seq, np.maximum(want.frame_state, 0).astype(np.int64), 1), -1)
        assert np.array_equal(_np(got.labels), lab)
        n_feasible += int((want.total != -np.inf).sum())
    assert n_feasible >= 4, n_feasible                               # (the long utterances at least)


def test_ragged_batch_alone_twice_inputs_and_fills():
    """Feasible, infeasible and zero-length utterances in one batch; an utterance alone (its own tight shapes: another K,
    another workspace) equals the same utterance in the batch; two runs are identical; the inputs are untouched; the
    regions beyond n_frames / n_seq hold exactly the defined fill, on output memory that held NaN before."""
    import evaluation as ev
    from conftest import poison_gpu_state
    rng = np.random.RandomState(11)
    Fmax, Smax, C = 140, 300, 61
    nf = np.array([140, 0, 33, 100, 17, 140, 1, 139, 64, 5], np.int32)
    ns = np.array([60, 10, 0, 300, 17, 129, 1, 65, 200, 9], np.int32)
    B = len(nf)
    seq = rng.randint(0, C, size=(B, Smax)).astype(np.int32)
    seq[0, 3] = 61                                                   # an out-of-range class on the device: -inf
    seq[5, 7] = -5
    opt = (rng.rand(B, Smax) < 0.3).astype(np.uint8)
    opt[0, 3] = opt[5, 7] = 1
    score = rng.standard_normal((B, Fmax, C)).astype(np.float32)
    for b in range(B):
        if nf[b]:
            score[b, :nf[b]] = _scores(KINDS[b % 3], int(nf[b]), C, seq[b, :max(ns[b], 1)], rng)
    want = ar.align_batch_f32(score, seq, opt, nf, ns)
    feas = want.total != -np.inf
    assert feas.sum() >= 4 and (~feas).sum() >= 4 and not feas[1] and not feas[2] and not feas[3]
    d_score, d_seq, d_opt = (torch.from_numpy(v).cuda() for v in (score, seq, opt))
    d_nf, d_ns = torch.from_numpy(nf).cuda(), torch.from_numpy(ns).cuda()
    poison_gpu_state()
    got = ev.align_batch(d_score, d_nf, d_seq, d_ns, optional=d_opt, kind='log')
    _assert_equal(got, want)
    for b in range(B):                                              # the fills, spelled out
        F, S = (int(nf[b]), int(ns[b])) if feas[b] else (0, 0)
        assert (_np(got.frame_state)[b, F:] == -1).all() and (_np(got.labels)[b, F:] == -1).all()
        assert (_np(got.start)[b, S:] == -1).all() and (_np(got.end)[b, S:] == -1).all() and np.isnan(_np(got.seg_score)[b, S:]).all()
    again = ev.align_batch(d_score, d_nf, d_seq, d_ns, optional=d_opt, kind='log')
    for k in INT_FIELDS + F32_FIELDS + ('labels',):
        a, b_ = _np(getattr(got, k)), _np(getattr(again, k))
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b_.view(np.uint32) if b_.dtype == np.float32 else b_), k
    assert np.array_equal(_np(d_score), score) and np.array_equal(_np(d_seq), seq) and np.array_equal(_np(d_opt), opt)
    assert np.array_equal(_np(d_nf), nf) and np.array_equal(_np(d_ns), ns)
    for b in (0, 3, 4, 5, 6, 7, 8):
        F, S = int(nf[b]), int(ns[b])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # (device arrays: seq is not range-checked)
        one = ev.align_batch(dev(score[b:b + 1, :F]), [F], dev(seq[b:b + 1, :S]), [S], optional=dev(opt[b:b + 1, :S]), kind='log')
        assert np.array_equal(_np(one.frame_state)[0], want.frame_state[b, :F]), b
        for k in ('start', 'end'):
            assert np.array_equal(_np(getattr(one, k))[0], getattr(want, k)[b, :S]), (b, k)
        assert np.array_equal(_canon(_np(one.seg_score)[0]), _canon(want.seg_score[b, :S])), b
        assert _canon(_np(one.total))[0] == _canon(want.total[b:b + 1])[0] and int(one.n_visited[0]) == want.n_visited[b], b


def test_path_cost_within_the_derived_bound_of_the_float64_optimum():
    """Non-integer scores: the device's path, re-costed in float64, against the float64 optimum.

    Bound.  Float32 addition is monotone (a >= b implies fl(e + a) >= fl(e + b)), so by induction over the frames the
    float32 recurrence returns the path p32 whose FLOAT32 cost V32 -- its emissions added in frame order, one rounding per
    addition -- is the greatest over all admissible paths; in particular V32 >= fl32(p*), the float32 cost of the float64
    optimum p*.  The float32 cost of ANY path differs from its exact cost by at most F - 1 roundings of partial sums, each
    at most u |partial sum|, u = 2^-24, and every partial sum is bounded by A (1 + u)^F with A = sum_t max_s |e(t, s)|.
    Hence cost(p*) - cost(p32) <= (cost(p*) - fl32(p*)) + (V32 - cost(p32)) <= 2 (F - 1) u A (1 + u)^F, and the float64
    re-costing adds at most 2 F 2^-53 A.  For F <= 2^16 both together stay below
        gap <= 2 F u A.
    The gap cannot be negative by more than the re-costing error (p* is optimal): gap >= -2 F 2^-53 A."""
    import evaluation as ev
    rng = np.random.RandomState(21)
    B, F, S, C = 8, 130, 40, 61
    seq = rng.randint(0, C, size=(B, S)).astype(np.int32)
    opt = (rng.rand(B, S) < 0.2).astype(np.uint8)
    score = np.stack([_scores(('logsoftmax', 'peaked')[b % 2], F, C, seq[b], rng) for b in range(B)])
    got = ev.align_batch(score, [F] * B, seq, [S] * B, optional=opt, kind='log')
    fs = _np(got.frame_state)
    worst = 0.0
    for b in range(B):
        best = ar.align_f64(score[b], seq[b], opt[b])
        assert np.isfinite(best.total) and (fs[b] >= 0).all()
        e = np.abs(ar.emissions(score[b].astype(np.float64), seq[b], np.float64))
        A = e.max(1).sum()
        gap = float(best.total - ar.path_cost_f64(score[b], seq[b], fs[b]))
        bound = 2 * F * 2.0 ** -24 * A
        print('utterance %d: float64 optimum %.6f, gap %.3e, bound %.3e' % (b, float(best.total), gap, bound))
        assert -2 * F * 2.0 ** -53 * A <= gap <= bound, (b, gap, bound)
        worst = max(worst, gap / bound)
    print('largest gap / bound: %.3e' % worst)


@pytest.fixture(scope='module')
def wav_case(f32_models):
    """content_wav_batch's posteriors of the ragged batch, and for every utterance a transcript read off them."""
    import evaluation as ev
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = ev.content_wav_batch(dec.encoder, wav, lens, wav, lens, c, window_batch=64)
    seg = ev.phn_segments_batch(r.ppg_a, r.len_a, min_run=3)
    S = int(min(int(seg.n_seg.max()), 200))
    seq = seg.labels[:, :S].contiguous()
    n_seq = seg.n_seg.clamp(max=S).contiguous()
    torch.cuda.synchronize()
    return dict(enc=dec.encoder, c=c, wav=wav, lens=lens, ppg=r.ppg_a, n_frames=r.len_a, seq=seq, n_seq=n_seq)


def test_public_calls_equal_the_reference_and_do_not_synchronise(wav_case):
    """align_batch(kind='prob') against the reference fed with the device's own logged scores; align_wav_batch against
    align_batch on content_wav_batch's posteriors (golden encoder checkpoint, synthetic speech); both under
    torch.cuda.set_sync_debug_mode('error')."""
    import evaluation as ev
    w = wav_case
    rng = np.random.RandomState(31)
    B, F, S, C = 4, 70, 12, 61
    ppg = np.zeros((B, F, C), np.float32)
    for b in range(B):
        p = ar.synthetic_posteriors(rng.randint(0, C, size=S), rng.randint(3, 7, size=S), C, seed=b)[:F]
        ppg[b, :len(p)] = p
    ppg[0, 5, :3] = 0.0                                             # below the floor
    nf, ns = [36, 70, 50, 1], [12, 12, 9, 1]
    seq = rng.randint(0, C, size=(B, S)).astype(np.int32)
    opt = (rng.rand(B, S) < 0.3).astype(np.uint8)
    d_ppg, d_wav = torch.from_numpy(ppg).cuda(), torch.from_numpy(w['wav']).cuda()
    calls = (lambda: ev.align_batch(d_ppg, nf, seq, ns, optional=opt, kind='prob', floor=1e-6),
             lambda: ev.align_wav_batch(w['enc'], d_wav, w['lens'], w['seq'], w['n_seq'], w['c']),
             lambda: ev.align_wav_batch(w['enc'], d_wav, w['lens'], w['seq'], w['n_seq'], w['c'], ppg=w['ppg']))
    for c in calls:
        c()
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        a, wv, wp = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    logged = _np(torch.log(d_ppg.clamp_min(1e-6)))
    assert np.isfinite(logged).all() and logged[0, 5, 0] < -13.0                  # the floor was applied
    _assert_equal(a, ar.align_batch_f32(logged, seq, opt, np.array(nf), np.array(ns)))
    assert int(a.n_visited.sum()) > 0
    # waveforms in
    assert torch.equal(wv.ppg, w['ppg']) and torch.equal(wv.n_frames, w['n_frames'])
    want = ev.align_batch(w['ppg'], w['n_frames'], w['seq'], w['n_seq'])
    assert bool((want.total > -np.inf).all()) and int(want.n_visited.min()) >= 1     # the transcript came from these posteriors
    for r in (wv, wp):
        for k in INT_FIELDS + ('labels',):
            assert torch.equal(getattr(r, k), getattr(want, k)), k
        for k in F32_FIELDS:
            assert np.array_equal(_canon(_np(getattr(r, k))), _canon(_np(getattr(want, k)))), k
    assert torch.equal(wp.ppg, w['ppg'])
    # every state of a transcript read off the posteriors with min_run = 3 is visited, in order
    n_seq = _np(w['n_seq'])
    assert np.array_equal(_np(want.n_visited), n_seq)


def test_graph_replay_with_new_contents_and_lengths():
    """The two launches captured on static buffers with the lengths in device tensors, replayed after other contents and
    other lengths were copied into the same buffers: equal to the eager public call.  The first call is outside the
    capture."""
    import evaluation as ev
    rng = np.random.RandomState(41)
    B, F, S, C = 5, 70, 130, 61

    def contents(nf, ns):
        seq = rng.randint(0, C, size=(B, S)).astype(np.int32)
        opt = (rng.rand(B, S) < 0.3).astype(np.uint8)
        score = rng.standard_normal((B, F, C)).astype(np.float32)
        for b in range(B):
            if nf[b]:
                score[b, :nf[b]] = _scores(KINDS[b % 4], nf[b], C, seq[b, :max(ns[b], 1)], rng)
        return score, seq, opt

    nf0, ns0 = [70, 33, 16, 64, 1], [20, 33, 5, 130, 1]
    h = contents(nf0, ns0)
    d_score, d_seq, d_opt = (torch.from_numpy(v).cuda() for v in h)
    d_nf, d_ns = torch.tensor(nf0, dtype=torch.int32, device='cuda'), torch.tensor(ns0, dtype=torch.int32, device='cuda')
    ev._align_launch(d_score, d_seq, d_opt, d_nf, d_ns)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = ev._align_launch(d_score, d_seq, d_opt, d_nf, d_ns)

    def check(h, nf, ns):
        g.replay()
        torch.cuda.synchronize()
        eager = ev.align_batch(h[0], nf, h[1], ns, optional=h[2], kind='log')
        want = ar.align_batch_f32(h[0], h[1], h[2], np.array(nf), np.array(ns))
        _assert_equal(out, want)
        for k in INT_FIELDS + ('labels',):
            assert torch.equal(getattr(out, k), getattr(eager, k)), k
        for k in F32_FIELDS:
            assert np.array_equal(_canon(_np(getattr(out, k))), _canon(_np(getattr(eager, k)))), k
        return want

    w0 = check(h, nf0, ns0)
    assert (w0.total != -np.inf).sum() >= 3
    nf1, ns1 = [17, 70, 0, 2, 69], [17, 65, 9, 2, 30]
    h1 = contents(nf1, ns1)
    for d, v in zip((d_score, d_seq, d_opt), h1):
        d.copy_(torch.from_numpy(v))
    d_nf.copy_(torch.tensor(nf1, dtype=torch.int32))
    d_ns.copy_(torch.tensor(ns1, dtype=torch.int32))
    w1 = check(h1, nf1, ns1)
    assert not np.array_equal(w0.frame_state, w1.frame_state)


def test_limits_raise_value_error():
    import evaluation as ev
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='1024'):
        ev.align_batch(z(1, 4, 3), [4], zi(1, 1025), [2])
    with pytest.raises(ValueError, match='65535'):
        ev.align_batch(z(1, 1, 65536), [1], zi(1, 1), [1])
    with pytest.raises(ValueError, match='65535'):
        ev.align_batch(np.broadcast_to(np.float32(0), (65536, 1, 1)), [1] * 65536, np.zeros((65536, 1), np.int32), [1] * 65536)
    with pytest.raises(ValueError, match='2 GiB'):
        ev.align_batch(np.broadcast_to(np.float32(0), (4000, 16384, 1)), [1] * 4000, zi(4000, 1024), [1] * 4000)
    r = ev.align_batch(z(1, 4, 3), [4], zi(1, 1024), [2], kind='log')        # at the limit: runs
    assert _np(r.frame_state).tolist() == [[0, 1, 1, 1]] and float(r.total[0]) == 0.0      # (stay is preferred: the advance is the forced one)
