"""Phone-loop decoding on the device (vc_decode_f32 behind evaluation.decode_batch) against the float32 restatement of
tests/decode_ref.py: every output bit for bit (the NaN padding of seg_score compared as NaN)."""
import numpy as np
import pytest
import torch

import align_ref as ar
import decode_ref as dr
from test_convert_batch_gpu import _ragged, f32_models        # noqa: F401  (a fixture and its inputs; that file is not edited)

pytestmark = pytest.mark.gpu

NEG = -np.inf
# the seams of M (1, 2, 3, 8), of the prefetch depth and of the 4-frame word of moves (3, 4, 5), of the walker's 64-frame ballot
# (63, 64, 65, 130); the two utterances of 300 frames give the back-track's lanes chunks of more than one frame (F > 256)
FRAMES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 63, 64, 65, 130)
LONG = 300
KINDS = ('int', 'logsoftmax', 'peaked', 'neginf')
TRANS = ('zeros', 'int', 'bigram', 'neginf')


def _np(t):
    return t.detach().cpu().numpy()


def _canon(x):
    """float32 bits with every NaN mapped to one pattern."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).copy()
    b[np.isnan(x)] = 0x7fc00000
    return b


def _assert_equal(got, want, cmap=None, what=''):
    assert np.array_equal(_np(got.frame_class), want.frame_class), (what, 'frame_class')
    lab = want.frame_class if cmap is None else np.where(want.frame_class >= 0, np.asarray(cmap)[np.maximum(want.frame_class, 0)], -1)
    assert np.array_equal(_np(got.labels), lab), (what, 'labels')
    for g, w in zip(got.seg, (want.seg_label, want.seg_start, want.seg_end, want.n_seg)):
        assert np.array_equal(_np(g), w), (what, 'seg')
    assert np.array_equal(_canon(_np(got.seg_score)), _canon(want.seg_score)), (what, 'seg_score')
    assert np.array_equal(_canon(_np(got.total)), _canon(want.total)), (what, 'total')
    assert np.array_equal(_np(got.feasible), want.total != NEG), (what, 'feasible')


def _log_softmax(x):
    x = x.astype(np.float32)
    m = x.max(-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)


def _speech(F, C, rng, noise=0.2):
    """Speech-like log-posteriors: random segments of 1 to 9 frames."""
    lens = []
    while sum(lens) < F:
        lens.append(int(rng.randint(1, 10)))
    p = ar.synthetic_posteriors(rng.randint(0, C, size=len(lens)), lens, C, seed=int(rng.randint(1 << 30)), peak=0.6, noise=noise)[:F]
    return np.log(np.maximum(p, np.float32(1e-10))).astype(np.float32)


def _scores(kind, F, C, rng):
    if kind == 'int':
        return rng.randint(-3, 1, size=(F, C)).astype(np.float32)
    if kind == 'peaked':
        return _speech(F, C, rng)
    x = _log_softmax(rng.standard_normal((F, C)) * 2.0)
    if kind == 'neginf':
        x[rng.rand(F, C) < 0.3] = NEG
        x[rng.rand(F) < 0.1] = NEG
    return x


def _trans(kind, C, rng):
    if kind == 'zeros':
        return np.zeros((C, C), np.float32)
    if kind == 'int':                                               # ties everywhere: this pins the tie rules
        return rng.randint(-2, 1, size=(C, C)).astype(np.float32)
    if kind == 'bigram':                                            # a -inf diagonal
        return dr.phn_transitions(rng.randint(0, C, size=(8, 40)), np.full(8, 40), C)
    t = rng.standard_normal((C, C)).astype(np.float32)
    t[rng.rand(C, C) < 0.3] = NEG
    return t


def _fold(C):
    """Pairs of classes folded onto the even one, every fifth class dropped."""
    m = (np.arange(C) // 2 * 2).astype(np.int32)
    m[::5] = -1
    return m


def _batch(C, seed):
    """Every F of FRAMES x every kind, plus two long utterances: (score, n_frames); rows beyond n_frames are NOT neutral."""
    rng = np.random.RandomState(seed)
    cases = [(F, k) for F in FRAMES for k in KINDS] + [(LONG, 'int'), (LONG, 'peaked')]
    score = rng.standard_normal((len(cases), LONG, C)).astype(np.float32)
    for b, (F, k) in enumerate(cases):
        score[b, :F] = _scores(k, F, C, rng)
    return score, np.array([F for F, _ in cases], np.int32)


@pytest.mark.parametrize('M', [1, 2, 3, 8])
@pytest.mark.parametrize('C', [1, 2, 61, 63, 64, 65, 127, 128])
def test_bit_exact_against_the_float32_reference(C, M):
    """F over the seams named at FRAMES x C over both kernel forms and their edges x M x four kinds of scores x four kinds
    of trans x init / final / class_map NULL and given: every output."""
    import evaluation as ev
    rng = np.random.RandomState(C * 11 + M)
    score, nf = _batch(C, seed=C * 7 + M)
    d_score, d_nf = torch.from_numpy(score).cuda(), torch.from_numpy(nf).cuda()
    n_feasible = 0
    for k, tk in enumerate(TRANS):
        trans = _trans(tk, C, rng)
        if k % 2 == 0:
            init = final = cmap = None
        else:
            init, final = (rng.randint(-2, 1, size=C).astype(np.float32) for _ in range(2))
            init[rng.randint(C)] = NEG if C > 2 else 0.0
            cmap = _fold(C)
        want = dr.decode_batch_f32(score, nf, trans, init, final, M, cmap)
        got = ev.decode_batch(d_score, d_nf, trans=trans, init=init, final=final, min_dur=M, class_map=cmap, kind='log')
        _assert_equal(got, want, cmap, tk)
        n_feasible += int((want.total != NEG).sum())
    assert n_feasible >= 40, n_feasible


def _ragged_case():
    rng = np.random.RandomState(11)
    Fmax, C, M = 140, 61, 3
    nf = np.array([140, 0, 33, 2, 17, 140, 1, 139, 64, 5, 100], np.int32)
    score = rng.standard_normal((len(nf), Fmax, C)).astype(np.float32)
    for b, F in enumerate(nf):
        if F:
            score[b, :F] = _scores(KINDS[b % 3], int(F), C, rng)
    score[10, :100] = NEG                                           # every path -inf
    return score, nf, _trans('bigram', C, rng), rng.randint(-2, 1, size=C).astype(np.float32), _fold(C), M


def test_ragged_batch_alone_twice_inputs_and_fills():
    """Zero-length, F < M and all -inf utterances between feasible ones; the outputs land on NaN-poisoned memory; the inputs
    are untouched; an utterance alone (its own F_max, batch size and workspace) equals itself in the batch; two calls agree."""
    import evaluation as ev
    from conftest import poison_gpu_state
    score, nf, trans, init, cmap, M = _ragged_case()
    want = dr.decode_batch_f32(score, nf, trans, init, None, M, cmap)
    feas = want.total != NEG
    assert feas.sum() >= 6 and not feas[1] and not feas[3] and not feas[6] and not feas[10]
    d = [torch.from_numpy(v).cuda() for v in (score, nf, trans, init, cmap)]
    poison_gpu_state()
    call = lambda: ev.decode_batch(d[0], d[1], trans=d[2], init=d[3], min_dur=M, class_map=d[4], kind='log')
    got = call()
    _assert_equal(got, want, cmap)
    for b in range(len(nf)):                                        # the fills, spelled out
        F, n = (int(nf[b]) if feas[b] else 0), int(want.n_seg[b])
        assert (_np(got.frame_class)[b, F:] == -1).all() and (_np(got.labels)[b, F:] == -1).all()
        assert all((_np(g)[b, n:] == -1).all() for g in got.seg[:3]) and np.isnan(_np(got.seg_score)[b, n:]).all()
        assert not np.isnan(_np(got.seg_score)[b, :n]).any()
    again = call()
    for a, b_ in zip((got.frame_class, got.labels, got.seg_score, got.total, *got.seg), (again.frame_class, again.labels, again.seg_score, again.total, *again.seg)):
        assert np.array_equal(_canon(_np(a)) if a.dtype == torch.float32 else _np(a), _canon(_np(b_)) if a.dtype == torch.float32 else _np(b_))
    for t, h in zip(d, (score, nf, trans, init, cmap)):
        assert np.array_equal(_np(t), h, equal_nan=True)
    for b in (0, 2, 4, 5, 7, 8, 9):
        F = int(nf[b])
        one = ev.decode_batch(np.ascontiguousarray(score[b:b + 1, :F]), [F], trans=trans, init=init, min_dur=M, class_map=cmap, kind='log')
        assert np.array_equal(_np(one.frame_class)[0], want.frame_class[b, :F]), b
        for g, w in zip(one.seg[:3], (want.seg_label, want.seg_start, want.seg_end)):
            assert np.array_equal(_np(g)[0], w[b, :F]), b
        assert np.array_equal(_canon(_np(one.seg_score)[0]), _canon(want.seg_score[b, :F])), b
        assert _canon(_np(one.total))[0] == _canon(want.total[b:b + 1])[0] and int(one.seg.n_seg[0]) == want.n_seg[b], b


def test_path_cost_within_the_derived_bound_of_the_float64_optimum():
    """Speech-like scores and a bigram matrix (a -inf diagonal, so the frames' classes determine the path): the device's
    path, re-costed in float64, against the float64 optimum (the restatement run in float64).

    Bound.  Float32 addition is monotone (a >= b implies fl(e + a) >= fl(e + b)), so by induction over the frames the
    float32 recurrence returns the path p32 whose FLOAT32 cost V32 -- its terms added in the recurrence's order, one
    rounding per addition -- is the greatest over all admissible paths; in particular V32 >= fl32(p*), the float32 cost of
    the float64 optimum p*.  Along a path every frame after the first costs at most two additions (the transition into a
    new segment, then the emission; one when the path stays), so the float32 cost of ANY path differs from its exact cost
    by at most 2 F roundings of partial sums, each at most u |partial sum|, u = 2^-24, and every partial sum is bounded
    by A (1 + u)^(2F) with A = sum over t of (max_c |e(t, c)| + max |trans|), the maxima over the finite entries.  Hence
        gap = cost(p*) - cost(p32) <= (cost(p*) - fl32(p*)) + (V32 - cost(p32)) <= 2 * 2 F u A (1 + u)^(2F),
    and the float64 re-costing adds at most 4 F 2^-53 A; for F <= 2^16 both together stay below  gap <= 4 F u A (1 + 2^-8).
    The gap cannot be negative by more than the re-costing error (p* is optimal): gap >= -4 F 2^-53 A."""
    import evaluation as ev
    rng = np.random.RandomState(21)
    B, F, C, M = 8, 130, 61, 3
    score = np.stack([_speech(F, C, rng, noise=(0.1, 0.4)[b % 2]) for b in range(B)])
    trans = dr.phn_transitions(rng.randint(0, C, size=(30, 50)), np.full(30, 50), C)
    got = ev.decode_batch(score, [F] * B, trans=trans, min_dur=M, kind='log')
    fc = _np(got.frame_class)
    worst = 0.0
    for b in range(B):
        best = dr.decode_f64(score[b], trans, min_dur=M)
        assert np.isfinite(best.total) and (fc[b] >= 0).all()
        A = np.abs(score[b].astype(np.float64)).max(1).sum() + F * float(np.abs(trans[np.isfinite(trans)]).max())
        gap = float(best.total - dr.path_cost_f64(score[b], trans, None, None, dr.raw_from_frames(fc[b])))
        bound = 4 * F * 2.0 ** -24 * A * (1 + 2.0 ** -8)
        print('utterance %d: float64 optimum %.6f, gap %.3e, bound %.3e' % (b, float(best.total), gap, bound))
        assert -4 * F * 2.0 ** -53 * A <= gap <= bound, (b, gap, bound)
        worst = max(worst, gap / bound)
    print('largest gap / bound: %.3e' % worst)


def _quality_batch(noise):
    from test_decode_cpu import _quality_case
    cases = [_quality_case(seed, noise) for seed in range(10)]
    Fmax = max(len(p) for _, p in cases)
    ppg = np.full((10, Fmax, 61), 1.0 / 61, np.float32)
    for b, (_, p) in enumerate(cases):
        ppg[b, :len(p)] = p
    return [labs for labs, _ in cases], ppg, np.array([len(p) for _, p in cases], np.int32)


def test_quality_case_on_the_device_and_content_batch_viterbi():
    """The CPU quality case decoded on the device: the same sequences as the restatement (at noise 0.02: the truth);
    content_batch(sequence='viterbi') on (clean, noisy) pairs returns the edit distance of the two decoded sequences."""
    import evaluation as ev
    truth, clean, nf = _quality_batch(0.02)
    _, noisy, nf2 = _quality_batch(0.4)
    assert np.array_equal(nf, nf2)
    z = np.zeros((61, 61), np.float32)
    dc, dn = (ev.decode_batch(p, nf, trans=z, min_dur=3) for p in (clean, noisy))
    logged = lambda p: _np(torch.log(torch.from_numpy(p).cuda().clamp_min(1e-10)))
    _assert_equal(dc, dr.decode_batch_f32(logged(clean), nf, z, min_dur=3))
    _assert_equal(dn, dr.decode_batch_f32(logged(noisy), nf, z, min_dur=3))
    for b in range(10):
        assert _np(dc.seg.labels)[b, :int(dc.seg.n_seg[b])].tolist() == truth[b], b
    r = ev.content_batch(clean, noisy, nf, nf, sequence='viterbi', decode=dict(min_dur=3))
    e = ev.edit_distance_batch(dc.seg.labels, dn.seg.labels, dc.seg.n_seg, dn.seg.n_seg)
    for k in ('dist', 'n_match', 'n_sub', 'n_del', 'n_ins'):
        assert torch.equal(getattr(r, k), getattr(e, k)), k
    assert torch.equal(r.seg_a.labels, dc.seg.labels) and torch.equal(r.seg_b.labels, dn.seg.labels) and torch.equal(r.seg_b.n_seg, dn.seg.n_seg)
    want = [dr.edit_distance(truth[b], _np(dn.seg.labels)[b, :int(dn.seg.n_seg[b])]) for b in range(10)]
    assert _np(r.dist).tolist() == want
    # the mask compaction comes first, as for the arg-max sequences
    mask = np.ones(clean.shape[:2], np.uint8)
    mask[:, 5:9] = 0
    rm = ev.content_batch(clean, noisy, nf, nf, sequence='viterbi', decode=dict(min_dur=3), mask_a=mask, mask_b=mask)
    keep = np.r_[0:5, 9:clean.shape[1]]
    dm = ev.decode_batch(np.ascontiguousarray(noisy[:, keep]), nf - 4, trans=z, min_dur=3)
    assert torch.equal(rm.seg_b.labels[:, :len(keep)], dm.seg.labels) and torch.equal(rm.seg_b.n_seg, dm.seg.n_seg)


def test_content_batch_default_is_unchanged():
    """content_batch with default arguments: bit for bit phn_segments_batch + edit_distance_batch + ppg_metrics_batch called
    separately."""
    import evaluation as ev
    _, clean, nf = _quality_batch(0.02)
    _, noisy, _ = _quality_batch(0.4)
    cmap = _fold(61)
    r = ev.content_batch(clean, noisy, nf, nf, class_map=cmap)
    sa, sb = ev.phn_segments_batch(clean, nf, class_map=cmap), ev.phn_segments_batch(noisy, nf, class_map=cmap)
    e = ev.edit_distance_batch(sa.labels, sb.labels, sa.n_seg, sb.n_seg)
    m = ev.ppg_metrics_batch(clean, noisy, nf, nf, class_map=cmap)
    for a, b in zip(r.seg_a + r.seg_b, sa + sb):
        assert torch.equal(a, b)
    for k in e._fields + m._fields:
        a, b = getattr(r, k), getattr(e if k in e._fields else m, k)
        assert np.array_equal(_canon(_np(a)), _canon(_np(b))) if a.dtype == torch.float32 else torch.equal(a, b), k
    assert int(r.dist.sum()) > 0


@pytest.fixture(scope='module')
def wav_case(f32_models):
    import evaluation as ev
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = ev.content_wav_batch(dec.encoder, wav, lens, wav, lens, c, window_batch=64)
    torch.cuda.synchronize()
    return dict(enc=dec.encoder, c=c, wav=wav, lens=lens, ppg=r.ppg_a, n_frames=r.len_a)


def test_public_calls_equal_the_reference_and_do_not_synchronise(wav_case):
    """decode_batch(kind='prob', penalty) against the reference fed with the device's own logged scores; decode_wav_batch
    against decode_batch on content_wav_batch's posteriors; content_wav_batch(sequence='viterbi'); all under
    torch.cuda.set_sync_debug_mode('error')."""
    import evaluation as ev
    w = wav_case
    rng = np.random.RandomState(31)
    B, F, C = 4, 70, 61
    ppg = np.exp(np.stack([_speech(F, C, rng) for _ in range(B)]))
    ppg[0, 5, :3] = 0.0                                             # below the floor
    nf = [36, 70, 50, 1]
    trans = _trans('bigram', C, rng)
    cmap = _fold(C)
    trans_w = _trans('bigram', int(w['ppg'].shape[2]), rng)          # (the encoder's own class count)
    d_ppg, d_wav, d_trans = torch.from_numpy(ppg).cuda(), torch.from_numpy(w['wav']).cuda(), torch.from_numpy(trans_w).cuda()
    calls = (lambda: ev.decode_batch(d_ppg, nf, trans=trans, penalty=-0.5, min_dur=2, class_map=cmap, floor=1e-6),
             lambda: ev.decode_batch(d_ppg, nf, penalty=-1.0, min_dur=1),
             lambda: ev.decode_wav_batch(w['enc'], d_wav, w['lens'], w['c'], trans=d_trans, min_dur=3),
             lambda: ev.decode_wav_batch(w['enc'], d_wav, w['lens'], w['c'], trans=d_trans, min_dur=3, ppg=w['ppg']),
             lambda: ev.content_wav_batch(w['enc'], d_wav, w['lens'], d_wav, w['lens'], w['c'], sequence='viterbi', decode=dict(trans=d_trans)))
    for c in calls:
        c()
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        a, p, wv, wp, cw = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    logged = _np(torch.log(d_ppg.clamp_min(1e-6)))
    assert np.isfinite(logged).all() and logged[0, 5, 0] < -13.0                  # the floor was applied
    _assert_equal(a, dr.decode_batch_f32(logged, nf, (trans + np.float32(-0.5)).astype(np.float32), None, None, 2, cmap), cmap)
    _assert_equal(p, dr.decode_batch_f32(_np(torch.log(d_ppg.clamp_min(1e-10))), nf, np.full((C, C), -1.0, np.float32), min_dur=1))
    assert int(a.seg.n_seg.sum()) > 0 and bool(a.feasible[:3].all())
    # waveforms in
    assert torch.equal(wv.ppg, w['ppg']) and torch.equal(wv.n_frames, w['n_frames']) and torch.equal(wp.ppg, w['ppg'])
    want = ev.decode_batch(w['ppg'], w['n_frames'], trans=trans_w, min_dur=3)
    assert bool(want.feasible.all()) and int(want.seg.n_seg.min()) >= 1
    for r in (wv, wp):
        for g, x in zip((r.frame_class, r.labels, *r.seg), (want.frame_class, want.labels, *want.seg)):
            assert torch.equal(g, x)
        for k in ('seg_score', 'total'):
            assert np.array_equal(_canon(_np(getattr(r, k))), _canon(_np(getattr(want, k)))), k
    assert torch.equal(cw.seg_a.labels, want.seg.labels) and torch.equal(cw.seg_a.n_seg, want.seg.n_seg)
    assert int(cw.dist.max()) == 0                                  # both sides are the same waveform
    # every decoded segment lasts min_dur frames: a pseudo-transcript that survives phn_v_from_alignment's round trip
    n = _np(want.seg.n_seg)
    dur = _np(want.seg.end) - _np(want.seg.start)
    assert all(dur[b, :n[b]].min() >= 3 for b in range(len(n)))


def test_graph_replay_with_new_contents_and_lengths():
    """The launches captured on static buffers with the lengths in a device tensor, replayed after other contents and other
    lengths were copied into the same buffers: equal to the eager public call.  The first call is outside the capture."""
    import evaluation as ev
    rng = np.random.RandomState(41)
    B, F, C, M = 5, 70, 65, 2

    def contents(nf):
        score = rng.standard_normal((B, F, C)).astype(np.float32)
        for b in range(B):
            if nf[b]:
                score[b, :nf[b]] = _scores(KINDS[b % 4], nf[b], C, rng)
        return score, _trans(TRANS[1 + len(nf) % 2], C, rng)

    nf0 = [70, 33, 16, 64, 1]
    h = contents(nf0)
    cmap = _fold(C)
    d_score, d_trans = (torch.from_numpy(v).cuda() for v in h)
    d_nf, d_cmap = torch.tensor(nf0, dtype=torch.int32, device='cuda'), torch.from_numpy(cmap).cuda()
    dec = ev._decode_args(d_trans, 0.0, None, None, M, 'log', 1e-10, C, 'test')
    ev._decode_launch(d_score, d_nf, d_cmap, dec)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = ev._decode_launch(d_score, d_nf, d_cmap, dec)

    def check(h, nf):
        g.replay()
        torch.cuda.synchronize()
        want = dr.decode_batch_f32(h[0], np.array(nf), h[1], None, None, M, cmap)
        _assert_equal(out, want, cmap)
        _assert_equal(ev.decode_batch(h[0], nf, trans=h[1], min_dur=M, class_map=cmap, kind='log'), want, cmap)
        return want

    w0 = check(h, nf0)
    assert (w0.total != NEG).sum() >= 3
    nf1 = [17, 70, 0, 2, 69]
    h1 = contents(nf1)
    for d, v in zip((d_score, d_trans), h1):
        d.copy_(torch.from_numpy(v))
    d_nf.copy_(torch.tensor(nf1, dtype=torch.int32))
    w1 = check(h1, nf1)
    assert not np.array_equal(w0.frame_class, w1.frame_class)


def test_limits_raise_value_error_and_the_c_entry_refuses():
    import _vc
    import evaluation as ev
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match='128'):
        ev.decode_batch(z(1, 4, 129), [4])
    for m in (0, 9):
        with pytest.raises(ValueError, match='min_dur'):
            ev.decode_batch(z(1, 4, 3), [4], min_dur=m)
    with pytest.raises(ValueError, match='16384'):
        ev.decode_batch(z(1, 16385, 2), [4])
    with pytest.raises(ValueError, match='trans'):
        ev.decode_batch(z(1, 4, 3), [4], trans=z(3, 4))
    with pytest.raises(ValueError, match='trans'):
        ev.decode_batch(z(1, 4, 3), [4], trans=torch.zeros((3, 3), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='2 GiB'):
        ev.decode_batch(np.broadcast_to(np.float32(0), (2000, 16384, 128)), [1] * 2000)
    lib = _vc.lib()
    buf = torch.zeros(4096, dtype=torch.int32, device='cuda')
    p = _vc.ptr(buf)

    def entry(B, F, C, M):
        return lib.vc_decode_f32(p, p, p, None, None, None, B, F, C, M, p, p, p, p, p, p, p, p, 1 << 20, _vc.current_stream())

    for shape in ((1, 4, 129, 3), (1, 4, 3, 0), (1, 4, 3, 9), (1, 16385, 2, 3), (65536, 4, 3, 3), (2000, 16384, 128, 3)):
        assert entry(*shape) == 4, shape                           # VC_ERR_UNSUPPORTED, before any launch
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0
    r = ev.decode_batch(z(1, 16, 128), [16], min_dur=8, kind='log')                 # at the limits: runs
    assert _np(r.frame_class).tolist() == [[0] * 16] and float(r.total[0]) == 0.0 and int(r.seg.n_seg[0]) == 1
