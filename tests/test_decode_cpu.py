"""Phone-loop decoding without a GPU: the float32 restatement of tests/decode_ref.py against a brute force over every
segmentation and labelling, its special cases (frame-wise arg-max, forced alignment), infeasible inputs, class_map, the
quality claim on synthetic speech, phn_transitions, the round trip through audio_lib.calc_PHN_target, and the exports."""
import os
import re

import numpy as np
import pytest

import align_ref as ar
import decode_ref as dr
from conftest import ROOT

NEG = -np.inf


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_reference_equals_brute_force():
    """Every F <= 6, C <= 3, M <= 3 with init, trans and final on a small integer grid (float32 is exact there): the total
    is the optimum over every segmentation into segments of at least M frames and every labelling; the returned path
    re-costs to the total and every one of its segments lasts at least M frames."""
    rng = np.random.RandomState(0)
    n_feasible = n_infeasible = 0
    for F in range(1, 7):
        for C in range(1, 4):
            for M in range(1, 4):
                for rep in range(4):
                    score = rng.randint(-3, 2, size=(F, C)).astype(np.float32)
                    trans = rng.randint(-2, 1, size=(C, C)).astype(np.float32)
                    init = rng.randint(-2, 1, size=C).astype(np.float32)
                    final = rng.randint(-2, 1, size=C).astype(np.float32)
                    if rep == 3:
                        trans[rng.rand(C, C) < 0.4] = NEG
                        init[rng.rand(C) < 0.3] = NEG
                    if rep == 2:
                        init = final = None
                    r = dr.decode_f32(score, trans, init, final, M)
                    best = dr.brute_force(score, trans, init, final, M)
                    assert _bits(r.total) == _bits(best), (F, C, M, rep)
                    if best == NEG:
                        n_infeasible += 1
                        assert r.n_seg == 0 and (r.frame_class == -1).all() and r.raw == []
                        continue
                    n_feasible += 1
                    assert np.float32(dr.path_cost_f64(score, trans, init, final, r.raw)) == r.total
                    assert all(e - s >= M for _, s, e in r.raw) and r.raw[0][1] == 0 and r.raw[-1][2] == F
                    assert all(a[2] == b[1] for a, b in zip(r.raw[:-1], r.raw[1:]))
    assert n_feasible > 100 and n_infeasible > 20, (n_feasible, n_infeasible)


def test_frame_wise_special_case():
    """trans = 0, M = 1, no init / final, integer scores: the total is the sum of the row maxima and every frame takes an
    arg-max of its row -- THE arg-max where the row has one (rows that are permutations), and the lowest-index one at
    the last frame.  Where a row has several maxima the recurrence's own tie order decides, stay before enter (the order
    the reduction to forced alignment below needs): a frame keeps the class of the frame after it when that class is
    among its maxima, and takes its lowest-index arg-max otherwise."""
    rng = np.random.RandomState(1)
    for F, C in ((1, 1), (7, 3), (40, 61), (33, 128)):
        z = np.zeros((C, C), np.float32)
        score = np.stack([rng.permutation(C) for _ in range(F)]).astype(np.float32) - 3.0      # no ties within a row
        r = dr.decode_f32(score, z, min_dur=1)
        assert np.array_equal(r.frame_class, score.argmax(1)) and r.total == score.max(1).sum()
        score = rng.randint(-4, 3, size=(F, C)).astype(np.float32)                              # ties in most rows
        r = dr.decode_f32(score, z, min_dur=1)
        assert r.total == score.max(1).sum()
        want = np.empty(F, np.int32)
        want[F - 1] = score[F - 1].argmax()
        for t in range(F - 2, -1, -1):
            want[t] = want[t + 1] if score[t, want[t + 1]] == score[t].max() else score[t].argmax()
        assert np.array_equal(r.frame_class, want)


@pytest.mark.parametrize('kind', ['int', 'real'])
def test_reduction_to_forced_alignment(kind):
    """A sequence of pairwise distinct classes, trans 0 on (seq[k], seq[k+1]) and -inf elsewhere, init / final 0 on the first /
    last class and -inf elsewhere, M = 1: the loop is the transcript's left-to-right chain, so total and frame labels equal
    align_ref's bit for bit -- on the integer grid (ties everywhere) only if stay is preferred over advance as there."""
    rng = np.random.RandomState(2)
    n = 0
    for F, S, C in ((1, 1, 3), (6, 3, 5), (12, 4, 4), (40, 9, 12), (30, 30, 61), (5, 6, 8)):
        for rep in range(5):
            seq = rng.permutation(C)[:S]
            score = rng.randint(-3, 1, size=(F, C)).astype(np.float32) if kind == 'int' else \
                np.log(ar.synthetic_posteriors(rng.randint(0, C, size=F), np.ones(F, int), C, seed=rep, noise=0.3))
            trans = np.full((C, C), NEG, np.float32)
            trans[seq[:-1], seq[1:]] = 0.0
            init, final = np.full(C, NEG, np.float32), np.full(C, NEG, np.float32)
            init[seq[0]] = final[seq[-1]] = 0.0
            r = dr.decode_f32(score, trans, init, final, 1)
            a = ar.align_f32(score, seq)
            assert _bits(r.total) == _bits(a.total), (F, S, C, rep)
            lab = np.where(a.frame_state >= 0, seq[np.maximum(a.frame_state, 0)], -1)
            assert np.array_equal(r.frame_class, lab), (F, S, C, rep)
            n += int(a.total != NEG)
    assert n >= 20


def test_infeasible():
    z = np.zeros((3, 3), np.float32)
    none = lambda r, F: r.total == NEG and r.n_seg == 0 and (r.frame_class == -1).all() and len(r.frame_class) == F and \
        (r.seg_label == -1).all() and (r.seg_start == -1).all() and (r.seg_end == -1).all() and np.isnan(r.seg_score).all()
    assert none(dr.decode_f32(np.zeros((4, 3), np.float32), z, min_dur=1, n_frames=0), 4)       # F = 0
    assert none(dr.decode_f32(np.zeros((2, 3), np.float32), z, min_dur=3), 2)                   # F < M
    assert dr.decode_f32(np.zeros((3, 3), np.float32), z, min_dur=3).total == 0.0               # F = M: one segment
    s = np.zeros((5, 3), np.float32)
    s[2] = NEG
    assert none(dr.decode_f32(s, z, min_dur=1), 5)                                              # a frame nobody can emit
    assert none(dr.decode_f32(np.zeros((5, 3), np.float32), z, init=np.full(3, NEG, np.float32), min_dur=2), 5)
    t = np.full((3, 3), NEG, np.float32)                                                         # no transition at all, and
    s = np.full((6, 3), NEG, np.float32)                                                         # no class lasts: no path
    s[:3, 0] = s[3:, 1] = 0.0
    assert none(dr.decode_f32(s, t, min_dur=2), 6)
    t[0, 1] = -1.0
    r = dr.decode_f32(s, t, min_dur=2)
    assert r.total == -1.0 and r.raw == [(0, 0, 3), (1, 3, 6)]


def test_class_map_merges_and_drops_and_scores_the_merged_segment():
    C = 4
    lab = np.repeat([0, 1, 0, 2, 3, 1], [3, 4, 3, 2, 5, 3])
    F = len(lab)
    rng = np.random.RandomState(3)
    score = (rng.rand(F, C).astype(np.float32) - 3.0)
    score[np.arange(F), lab] = -rng.rand(F).astype(np.float32) * 0.1
    z = np.zeros((C, C), np.float32)
    r = dr.decode_f32(score, z, min_dur=2)
    assert np.array_equal(r.frame_class[:F], lab) and r.n_seg == 6
    # a b a with b -> -1 stays two a; 2 and 3 fold onto 2 and merge
    m = dr.decode_f32(score, z, min_dur=2, class_map=np.array([0, -1, 2, 2], np.int32))
    assert np.array_equal(m.frame_class, r.frame_class)
    assert m.n_seg == 3 and m.seg_label[:3].tolist() == [0, 0, 2] and m.seg_start[:3].tolist() == [0, 7, 10] and m.seg_end[:3].tolist() == [3, 10, 17]
    assert (m.seg_label[3:] == -1).all() and (m.seg_start[3:] == -1).all() and (m.seg_end[3:] == -1).all() and np.isnan(m.seg_score[3:]).all()
    want = np.float32(score[np.arange(10, 17), lab[10:17]].astype(np.float64).sum() / 7.0)
    assert _bits(m.seg_score[2]) == _bits(want)
    # two equal raw neighbours (a phoneme said twice) merge as well: the diagonal of trans is an ordinary entry
    s2 = np.full((6, 2), -5.0, np.float32)
    s2[:, 0] = 0.0
    t2 = np.array([[1.0, NEG], [NEG, NEG]], np.float32)
    r2 = dr.decode_f32(s2, t2, min_dur=2)
    assert r2.raw == [(0, 0, 2), (0, 2, 4), (0, 4, 6)] and r2.total == 2.0 and r2.n_seg == 1 and r2.seg_end[0] == 6


def _quality_case(seed, noise, C=61, n_seg=30):
    rng = np.random.RandomState(1000 + seed)
    labs = [int(rng.randint(C))]
    while len(labs) < n_seg:
        c = int(rng.randint(C))
        if c != labs[-1]:
            labs.append(c)
    lens = rng.randint(3, 12, size=n_seg)
    return labs, ar.synthetic_posteriors(labs, lens, C, seed=seed, peak=0.5, noise=noise)


def test_quality_on_synthetic_speech():
    """61 classes, 30 segments of 3 to 11 frames without immediate repeats, peak 0.5, seeds 0 to 9, trans = 0, M = 3: at
    noise 0.4 the summed edit distance of the decoded sequences to the truth is at most half that of the arg-max /
    min_run = 3 read-out; at noise 0.02 it is exactly 0."""
    z = np.zeros((61, 61), np.float32)
    for noise in (0.4, 0.02):
        dec = arg = 0
        for seed in range(10):
            labs, p = _quality_case(seed, noise)
            r = dr.decode_f32(np.log(np.maximum(p, np.float32(1e-10))), z, min_dur=3)
            dec += dr.edit_distance(labs, r.seg_label[:r.n_seg])
            arg += dr.edit_distance(labs, [s[0] for s in dr.argmax_segments(p, 3)])
        print('noise %.2f: decoder %d edit errors in 300 symbols, arg-max / min_run 3 %d' % (noise, dec, arg))
        if noise == 0.02:
            assert dec == 0
        else:
            assert 2 * dec <= arg and arg > 0, (dec, arg)


def test_phn_transitions():
    import evaluation as ev
    seqs = np.array([[0, 1, 2, 1, 9], [2, 2, 0, 9, 9]])
    t = ev.phn_transitions(seqs, [4, 3], 3, allow_repeat=True)
    # by hand: 0->1, 1->2, 2->1, 2->2, 2->0: rows (0 1 0), (0 0 1), (1 1 1) with add 1 over row total + 3
    want = np.log(np.array([[1, 2, 1], [1, 1, 2], [2, 2, 2]], np.float64) / np.array([[4.0], [4.0], [6.0]])).astype(np.float32)
    assert t.dtype == np.float32 and np.array_equal(t, want)
    assert np.allclose(np.exp(t.astype(np.float64)).sum(1), 1.0, atol=1e-6)
    rng = np.random.RandomState(4)
    seqs = rng.randint(0, 61, size=(20, 40))
    n = rng.randint(0, 41, size=20)
    for kw in (dict(allow_repeat=True), dict(add=0.5, scale=2.0), dict()):
        got = ev.phn_transitions(seqs, n, 61, **kw)
        assert np.array_equal(got, dr.phn_transitions(seqs, n, 61, **kw))
    assert np.allclose(np.exp(ev.phn_transitions(seqs, n, 61, allow_repeat=True).astype(np.float64)).sum(1), 1.0, atol=1e-5)
    d = ev.phn_transitions(seqs, n, 61)
    assert (np.diag(d) == NEG).all() and np.isfinite(d[~np.eye(61, dtype=bool)]).all()
    with pytest.raises(ValueError):
        ev.phn_transitions(np.array([[0, 3]]), [2], 3)
    with pytest.raises(ValueError):
        ev.phn_transitions(np.array([[0, 1]]), [3], 3)


def test_round_trip_through_calc_phn_target():
    """Decoded with min_dur = alignment_min_frames(80, 400), phn_v_from_alignment(seg_start, seg_end, seg_label) ->
    audio_lib.calc_PHN_target gives back the decoded labels frame for frame, on noisy posteriors where the arg-max read-out
    has shorter runs."""
    import audio_lib
    import evaluation as ev
    hop, W, C = 80, 400, 61
    M = ev.alignment_min_frames(hop, W)
    assert M == 3
    names = ['p%d' % i for i in range(C)]
    z = np.zeros((C, C), np.float32)
    for seed in range(4):
        _, p = _quality_case(seed, 0.4)
        F = len(p)
        assert min(b - a for _, a, b in dr.raw_from_frames(p.argmax(1))) < M
        r = dr.decode_f32(np.log(p), z, min_dur=M)
        for extra in (0, hop - 1):
            n_samples = (F - 1) * hop + extra
            phn_v = ev.phn_v_from_alignment(r.seg_start, r.seg_end, r.seg_label, names, hop, n_samples)
            assert len(phn_v) == r.n_seg
            got = audio_lib.calc_PHN_target(np.zeros(n_samples, np.float32), phn_v, {n: i for i, n in enumerate(names)}, hop, W)
            assert np.array_equal(got, r.frame_class[:F]), seed


def test_exports_in_header_table_and_library():
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    lib = _vc.lib()
    for name in ('vc_decode_workspace_bytes', 'vc_decode_f32'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _vc._SIGS and hasattr(lib, name)
    assert '/* Decoding.' in hdr
    q = lib.vc_decode_workspace_bytes
    a256 = lambda v: (v + 255) // 256 * 256
    assert q(16, 1000, 61) == a256(16 * 4) + a256(16 * 61 * 250 * 4)
    assert q(1, 1, 1) == 512 and q(0, 10, 10) == 0 and q(65536, 10, 10) == 0 and q(1, 10, 129) == 0 and q(1, 16385, 1) == 0
    assert q(1, 16384, 128) > 0 and q(65535, 16384, 128) == 0


def test_python_checks_come_before_the_gpu():
    """The argument checks of decode_batch and of content_batch's new arguments raise ValueError without a device."""
    import evaluation as ev
    p = np.full((1, 4, 3), 1 / 3, np.float32)
    for kw in (dict(min_dur=0), dict(min_dur=9), dict(min_dur=2.0), dict(trans=np.zeros((3, 2), np.float32)), dict(trans=np.zeros((3, 3))),
               dict(init=np.zeros(4, np.float32)), dict(final=np.full(3, np.nan, np.float32)), dict(trans=np.full((3, 3), np.inf, np.float32)),
               dict(penalty=float('nan')), dict(kind='logits'), dict(class_map=[0, 1, 3])):
        with pytest.raises(ValueError):
            ev.decode_batch(p, [4], **kw)
    with pytest.raises(ValueError, match='128'):
        ev.decode_batch(np.zeros((1, 2, 129), np.float32), [2])
    with pytest.raises(ValueError, match='16384'):
        ev.decode_batch(np.broadcast_to(np.float32(0), (1, 16385, 2)), [2])
    with pytest.raises(ValueError, match='sequence'):
        ev.content_batch(p, p, [4], [4], sequence='beam')
    with pytest.raises(ValueError, match='decode'):
        ev.content_batch(p, p, [4], [4], decode=dict(min_dur=2))
    with pytest.raises(ValueError, match='decode takes'):
        ev.content_batch(p, p, [4], [4], sequence='viterbi', decode=dict(min_run=2))
    with pytest.raises(ValueError, match='min_dur'):
        ev.content_batch(p, p, [4], [4], sequence='viterbi', decode=dict(min_dur=0))
