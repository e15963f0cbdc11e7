"""Forced alignment without a GPU: the float32 restatement of tests/align_ref.py against a brute force over every
admissible path, hand-made cases, recovery of a known segmentation, the round trip through audio_lib.calc_PHN_target,
the exports, and the argument checks of the Python calls."""
import itertools
import os
import re

import numpy as np
import pytest

import align_ref as ar
from conftest import ROOT

NEG = -np.inf


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------- reference against brute force
def test_reference_equals_brute_force_and_its_tie_choice():
    """Every F <= 6, S <= 4 and every opt pattern, on small-integer scores (exact sums, frequent ties): the total is the
    optimum over all admissible paths and the path is the one the strict compares prefer among the optimal ones; an empty
    set of admissible paths is reported infeasible."""
    rng = np.random.RandomState(0)
    n_feasible = n_infeasible = n_tied = 0
    for F in range(1, 7):
        for S in range(1, 5):
            for opt in itertools.product((0, 1), repeat=S):
                for rep in range(6):
                    C = 3
                    score = rng.randint(-2, 1, size=(F, C)).astype(np.float32)
                    seq = rng.randint(0, C, size=S).astype(np.int32)
                    got = ar.align_f32(score, seq, np.array(opt, np.uint8))
                    best, paths = ar.brute_force(score, seq, opt)
                    if not paths:
                        n_infeasible += 1
                        assert got.total == NEG and got.n_visited == 0 and (got.frame_state == -1).all()
                        assert (got.start == -1).all() and (got.end == -1).all() and np.isnan(got.seg_score).all()
                        continue
                    n_feasible += 1
                    n_tied += len(paths) > 1
                    assert got.total == best, (F, S, opt)
                    assert got.frame_state.tolist() == ar.tie_choice(paths, S), (F, S, opt, score, seq)
                    assert list(got.frame_state) in paths
    assert n_feasible > 500 and n_infeasible > 50 and n_tied > 100, (n_feasible, n_infeasible, n_tied)


def test_outputs_follow_from_the_path():
    """start / end / seg_score / n_visited restate frame_state; the float64 form agrees on integer scores."""
    rng = np.random.RandomState(1)
    for _ in range(50):
        F, S, C = rng.randint(1, 30), rng.randint(1, 9), 5
        score = rng.randint(-3, 1, size=(F, C)).astype(np.float32)
        seq = rng.randint(0, C, size=S).astype(np.int32)
        opt = (rng.rand(S) < 0.4).astype(np.uint8)
        r, r64 = ar.align_f32(score, seq, opt), ar.align_f64(score, seq, opt)
        assert float(r.total) == float(r64.total) and np.array_equal(r.frame_state, r64.frame_state)
        if r.total == NEG:
            continue
        fs = r.frame_state
        assert (np.diff(fs) >= 0).all() and (np.diff(fs) <= 2).all()
        for s in range(S):
            at = np.nonzero(fs == s)[0]
            if len(at) == 0:
                assert r.start[s] == -1 and r.end[s] == -1 and np.isnan(r.seg_score[s]) and opt[s]
            else:
                assert r.start[s] == at[0] and r.end[s] == at[-1] + 1
                assert r.seg_score[s] == np.float32(score[at, seq[s]].astype(np.float64).sum() / len(at))
        assert r.n_visited == len(set(fs.tolist()))
        assert float(r.total) == float(ar.path_cost_f64(score, seq, fs))


# ------------------------------------------------------------------------------------------------------------ hand-made cases
def _onehot_log(labels, C, hit=0.0, miss=-5.0):
    x = np.full((len(labels), C), miss, np.float32)
    x[np.arange(len(labels)), labels] = hit
    return x


def test_forced_diagonal():
    score = np.random.RandomState(2).standard_normal((5, 4)).astype(np.float32)
    seq = np.array([3, 1, 0, 2, 1], np.int32)
    r = ar.align_f32(score, seq)
    assert r.frame_state.tolist() == [0, 1, 2, 3, 4] and r.start.tolist() == [0, 1, 2, 3, 4] and r.end.tolist() == [1, 2, 3, 4, 5]
    want = np.float32(score[0, 3])
    for t in range(1, 5):
        want = np.float32(score[t, seq[t]] + want)
    assert _bits(r.total) == _bits(want) and r.n_visited == 5
    assert np.array_equal(_bits(r.seg_score), _bits(score[np.arange(5), seq]))


def test_fewer_frames_than_mandatory_states_is_infeasible():
    score = np.zeros((3, 4), np.float32)
    seq = np.array([0, 1, 2, 3, 0], np.int32)
    assert ar.align_f32(score, seq).total == NEG
    opt = np.array([0, 1, 0, 0, 0], np.uint8)                       # one optional: still 4 mandatory states for 3 frames
    r = ar.align_f32(score, seq, opt)
    assert r.total == NEG and (r.frame_state == -1).all() and r.n_visited == 0
    opt = np.array([0, 1, 0, 1, 0], np.uint8)                       # two optional, not adjacent: 3 mandatory, feasible
    r = ar.align_f32(score, seq, opt)
    assert r.total == 0 and r.frame_state.tolist() == [0, 2, 4] and r.start.tolist() == [0, -1, 1, -1, 2]
    assert ar.align_f32(score, seq, n_frames=0).total == NEG and ar.align_f32(score, seq, n_seq=0).total == NEG


@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_an_optional_state_taken_and_skipped(where):
    C = 4
    seq = {'first': [3, 0, 1, 2], 'middle': [0, 1, 3, 2], 'last': [0, 1, 2, 3]}[where]
    k = seq.index(3)
    opt = np.zeros(4, np.uint8)
    opt[k] = 1
    said_with = np.repeat(seq, 3)
    said_without = np.repeat([c for c in seq if c != 3], 3)
    r = ar.align_f32(_onehot_log(said_with, C), np.array(seq, np.int32), opt)
    assert r.frame_state.tolist() == np.repeat(np.arange(4), 3).tolist() and r.n_visited == 4 and r.total == 0
    r = ar.align_f32(_onehot_log(said_without, C), np.array(seq, np.int32), opt)
    others = [s for s in range(4) if s != k]
    assert r.frame_state.tolist() == np.repeat(others, 3).tolist() and r.n_visited == 3 and r.total == 0
    assert r.start[k] == -1 and r.end[k] == -1 and np.isnan(r.seg_score[k])
    assert [int(r.start[s]) for s in others] == [0, 3, 6] and [int(r.end[s]) for s in others] == [3, 6, 9]
    # without the mark the same audio has to pass through the state: one frame at the miss score, by the tie rule the first
    r = ar.align_f32(_onehot_log(said_without, C), np.array(seq, np.int32))
    assert r.n_visited == 4 and r.total == -5 and r.end[k] - r.start[k] == 1


def test_two_consecutive_optional_states_only_one_may_be_skipped():
    """seq 0 [1] [2] 3 with 1 and 2 optional, audio says 0 0 3 3: a skip passes over ONE state, chains are not built, so
    one of the two optional states takes a frame at the miss score; which one is the tie rule's choice."""
    seq = np.array([0, 1, 2, 3], np.int32)
    opt = np.array([0, 1, 1, 0], np.uint8)
    r = ar.align_f32(_onehot_log([0, 0, 3, 3], 4), seq, opt)
    assert r.total == -5 and r.n_visited == 3
    assert (r.start[1] == -1) != (r.start[2] == -1)
    best, paths = ar.brute_force(_onehot_log([0, 0, 3, 3], 4), seq, opt)
    assert best == -5 and r.frame_state.tolist() == ar.tie_choice(paths, 4)
    assert [0, 0, 3, 3] not in paths                                # the chain of two skips is not admissible
    # three frames: 0, then one optional state, then 3 is the only way
    r = ar.align_f32(_onehot_log([0, 3, 3], 4), seq, opt)
    assert r.total == -5 and r.n_visited == 3


def test_out_of_range_class_minus_inf_columns_and_nan():
    rng = np.random.RandomState(3)
    score = -rng.rand(6, 3).astype(np.float32)
    # a class outside [0, C) scores -inf: mandatory -> infeasible; optional -> skipped
    for bad in (-1, 3, 2 ** 31 - 1, -2 ** 31):
        seq = np.array([0, bad, 2], np.int64).astype(np.int32)
        assert ar.align_f32(score, seq).total == NEG
        r = ar.align_f32(score, seq, np.array([0, 1, 0], np.uint8))
        assert np.isfinite(r.total) and r.start[1] == -1 and r.n_visited == 2
    # a -inf column: the same
    s2 = score.copy()
    s2[:, 1] = NEG
    assert ar.align_f32(s2, np.array([0, 1, 2], np.int32)).total == NEG
    r = ar.align_f32(s2, np.array([0, 1, 2], np.int32), np.array([0, 1, 0], np.uint8))
    assert np.isfinite(r.total) and r.start[1] == -1
    # -inf at single frames steers the boundary
    s3 = np.zeros((6, 2), np.float32)
    s3[:4, 1] = NEG
    s3[4:, 0] = NEG
    assert ar.align_f32(s3, np.array([0, 1], np.int32)).frame_state.tolist() == [0, 0, 0, 0, 1, 1]
    # a NaN frame: comparisons with NaN are false, the total is NaN, NOT infeasible, and the walk is mechanical
    s4 = np.zeros((5, 2), np.float32)
    s4[2] = np.nan
    r = ar.align_f32(s4, np.array([0, 1], np.int32))
    assert np.isnan(r.total) and r.n_visited >= 1 and (r.frame_state >= 0).all() and (np.diff(r.frame_state) >= 0).all()
    again = ar.align_f32(s4, np.array([0, 1], np.int32))
    assert np.array_equal(r.frame_state, again.frame_state) and np.array_equal(r.start, again.start)


# ------------------------------------------------------------------------------------------- a known segmentation is recovered
SYN = dict(seed=5, peak=0.9, smooth=2, noise=0.02)


def synthetic_case(seed=SYN['seed']):
    """(posteriors [F, 61], seq, opt, true segment lengths): 40 segments of 4 .. 12 frames, neighbours differ; every
    fifth state is optional and two of those are absent from the audio."""
    rng = np.random.RandomState(seed)
    S, C = 40, 61
    seq = [int(rng.randint(C))]
    while len(seq) < S:
        c = int(rng.randint(C))
        if c != seq[-1] and (len(seq) < 2 or c != seq[-2]):
            seq.append(c)
    lens = rng.randint(4, 13, size=S)
    opt = np.zeros(S, np.uint8)
    opt[4::5] = 1
    lens[[9, 24]] = 0
    present = lens > 0
    ppg = ar.synthetic_posteriors(np.array(seq)[present], lens[present], C, **dict(SYN, seed=seed))
    return ppg, np.array(seq, np.int32), opt, lens


def test_synthetic_posteriors_recover_the_boundaries():
    """Smoothed one-hot posteriors plus noise: the box of 5 frames is symmetric, so the two neighbours' posteriors cross
    exactly at the true boundary; noise 0.02 against a step of (0.9 - 0.1 / 60) / 5 per frame cannot move it."""
    ppg, seq, opt, lens = synthetic_case()
    r = ar.align_f32(np.log(np.maximum(ppg, np.float32(1e-10))), seq, opt)
    edges = np.concatenate([[0], np.cumsum(lens)])
    for s in range(len(seq)):
        if lens[s] == 0:
            assert r.start[s] == -1 and r.end[s] == -1
        else:
            assert (r.start[s], r.end[s]) == (edges[s], edges[s + 1]), s
    assert r.n_visited == 38 and np.isfinite(r.total)


# ----------------------------------------------------------------------------------- round trip through calc_PHN_target
def _round_trip(seg_lens, hop, W, extra=0):
    import audio_lib
    import evaluation as ev
    S = len(seg_lens)
    names = ['p%d' % i for i in range(S)]
    seq = np.arange(S)
    edges = np.concatenate([[0], np.cumsum(seg_lens)])
    F = int(edges[-1])
    n_samples = (F - 1) * hop + extra
    labels = np.repeat(seq, seg_lens)
    phn_v = ev.phn_v_from_alignment(edges[:-1], edges[1:], seq, names, hop, n_samples)
    got = audio_lib.calc_PHN_target(np.zeros(n_samples, np.float32), phn_v, {n: i for i, n in enumerate(names)}, hop, W)
    assert len(got) == F
    return np.array_equal(got, labels)


@pytest.mark.parametrize('hop,W', [(80, 400), (40, 400), (160, 400), (80, 512), (1, 400), (3, 10), (200, 400), (512, 400)])
def test_phn_v_round_trip_holds_from_L_frames_and_not_below(hop, W):
    import evaluation as ev
    L = ev.alignment_min_frames(hop, W)
    assert L == (W // 2) // hop + 1
    rng = np.random.RandomState(hop + W)
    assert _round_trip([L] * 12, hop, W) and _round_trip([L] * 12, hop, W, extra=hop - 1)
    for _ in range(20):
        assert _round_trip((L + rng.randint(0, 4, size=rng.randint(2, 15))).tolist(), hop, W, extra=int(rng.randint(hop)))
    if L > 1:
        assert not _round_trip([L - 1] * 12, hop, W)                # the counter-example of the docstring
    assert ev.alignment_min_frames(80, 400) == 3


def test_phn_v_leaves_skipped_states_out_and_checks_its_arguments():
    import evaluation as ev
    v = ev.phn_v_from_alignment([0, -1, 5], [5, -1, 9], [7, 8, 9], {7: 'a', 8: 'pau', 9: 'b'}, 80, 700)
    assert v == [(0, 5 * 80 - 40, 'a'), (5 * 80 - 40, 700, 'b')]
    assert ev.phn_v_from_alignment([-1], [-1], [3], ['x'] * 4, 80, 700) == []
    with pytest.raises(ValueError):
        ev.phn_v_from_alignment([0], [5, 6], [1], ['x'] * 2, 80, 700)
    with pytest.raises(ValueError):
        ev.phn_v_from_alignment([0], [5], [1], ['x'] * 2, 0, 700)


# ------------------------------------------------------------------------------------------------------------------- exports
def test_exports_in_header_table_and_library():
    import ctypes
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    lib = _vc.lib()
    for name in ('vc_align_workspace_bytes', 'vc_align_f32'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _vc._SIGS and hasattr(lib, name)
    assert '/* Alignment.' in hdr
    q = lib.vc_align_workspace_bytes
    a256 = lambda v: (v + 255) // 256 * 256
    assert q(16, 1000, 300) == a256(16 * 4) + a256(16 * 63 * 300 * 4)
    assert q(1, 1, 1) == 512 and q(0, 10, 10) == 0 and q(65536, 10, 10) == 0 and q(1, 10, 1025) == 0 and q(1, 10, 0) == 0
    assert q(1, 2 ** 31 - 1, 1) > 0 and q(1, 2 ** 31 - 1, 4) == 0 and q(65535, 16384, 1024) == 0       # 2 GiB
    # argument errors of the C call come before any HIP call
    f = lib.vc_align_f32
    p = ctypes.c_void_p(4096)
    ok = dict(score=p, seq=p, opt=None, nf=p, ns=p, B=1, F=10, S=10, C=61, fs=p, st=p, en=p, sg=p, tot=p, nv=p, ws=p, wb=1 << 20, stream=None)
    call = lambda **kw: f(*dict(ok, **kw).values())
    for k in ('score', 'seq', 'nf', 'ns', 'fs', 'st', 'en', 'sg', 'tot', 'nv', 'ws'):
        assert call(**{k: None}) == 1 and b'vc_align_f32: NULL' in lib.vc_last_error(), k
    for kw in (dict(B=0), dict(F=0), dict(S=0), dict(C=0)):
        assert call(**kw) == 1 and b'vc_align_f32: bad shape' in lib.vc_last_error(), kw
    for kw in (dict(B=65536), dict(S=1025), dict(C=65536), dict(B=65535, F=16384, S=1024)):
        assert call(**kw) == 4 and b'vc_align_f32: limits' in lib.vc_last_error(), kw
    assert call(wb=100) == 3 and b'needed' in lib.vc_last_error()
    assert call(ws=ctypes.c_void_p(4097)) == 1 and b'unaligned' in lib.vc_last_error()


# ----------------------------------------------------------------------------------------------- Python argument errors
def test_python_argument_errors_come_before_any_gpu_use(monkeypatch):
    import torch
    import _vc
    import evaluation as ev

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched before the argument check')
    monkeypatch.setattr(ev, '_need_gpu', no_gpu)
    monkeypatch.setattr(ev, '_align_launch', no_gpu)
    B, F, C, S = 2, 20, 61, 5
    ppg = np.full((B, F, C), 1.0 / C, np.float32)
    seq = np.zeros((B, S), np.int32)
    good = dict(ppg=ppg, lens=[20, 10], seq=seq, n_seq=[5, 3])
    bad = [dict(ppg=ppg[0]), dict(ppg=ppg.astype(np.float64)), dict(ppg=np.zeros((B, F, 65536), np.float32)),
           dict(lens=[20]), dict(lens=[21, 1]), dict(lens=[-1, 1]), dict(lens=[1.5, 2.0]),
           dict(seq=seq[0]), dict(seq=seq.astype(np.int64)), dict(seq=np.zeros((3, S), np.int32)), dict(seq=np.zeros((B, 1025), np.int32)),
           dict(seq=np.full((B, S), 61, np.int32)), dict(seq=np.full((B, S), -1, np.int32)),
           dict(n_seq=[6, 1]), dict(n_seq=[1]), dict(n_seq=[-1, 1]),
           dict(optional=np.zeros((B, S + 1), np.uint8)), dict(optional=np.zeros((B, S), np.int32)),
           dict(kind='logit'), dict(floor=0.0), dict(floor=float('nan')), dict(floor=-1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            ev.align_batch(**dict(good, **kw))
    # an out-of-range class beyond the row's own count is padding, not an error; the limits come before the GPU as well
    pad = seq.copy()
    pad[1, 3:] = -1
    with pytest.raises(AssertionError, match='touched'):
        ev.align_batch(**dict(good, seq=pad))
    with pytest.raises(ValueError, match='2 GiB'):
        ev.align_batch(np.broadcast_to(np.float32(0), (4000, 16384, 1)), [1] * 4000, np.zeros((4000, 1024), np.int32), [1] * 4000)
    # align_wav_batch
    class Enc:
        cfg_d = {'n_output': 61}
    from test_convert_batch_cpu import CFG
    wav = np.zeros((2, 16000), np.float32)
    gw = dict(encoder=Enc(), wav=wav, lens=[16000, 9000], seq=seq, n_seq=[5, 3], cfg_d=CFG)
    badw = [dict(cfg_d=None), dict(wav=wav[0]), dict(lens=[16000]), dict(lens=[16001, 1]), dict(lens=[16000, 100]),
            dict(res_type='no_such'), dict(window_batch=0), dict(seq=np.full((B, S), 61, np.int32)), dict(n_seq=[6, 1]),
            dict(optional=np.zeros((B, S + 1), np.uint8)), dict(ppg=np.zeros((2, 7, 61), np.float32)),
            dict(seq=np.zeros((B, 1025), np.int32))]
    for kw in badw:
        with pytest.raises(ValueError):
            ev.align_wav_batch(**dict(gw, **kw))
    monkeypatch.undo()
    if not torch.cuda.is_available():
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            ev.align_batch(**good)
