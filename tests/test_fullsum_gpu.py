"""Full-sum alignment on the device (vc_fullsum_f32 behind evaluation.align_posterior_batch and
EncoderTrainer.forward_backward_transcript) against the float64 restatement of tests/fullsum_ref.py.

The bound, BOUND(F) = K_BOUND F 2^-24 absolute with K_BOUND = 64, on gamma, Gamma and log_z (occ: F times it), from the
roundings of csrc/vc_fullsum.hip as written.  u = 2^-24.  An error d in a log-domain value moves what is computed from it
by at most d (lse has non-negative partial derivatives that sum to 1), so errors add along the frames and never grow.
One frame of the forward recurrence, per cell: fs_lse3 subtracts the maximum from the two other terms (2 roundings of
d = x - m, each u |d|, which reaches the result weighted by exp(d): u |d| exp(-|d|) <= 0.37 u), takes two __expf (the
maximum's own term is exp(0) = 1 exactly; a product by log2(e) and a v_exp_f32 of one ulp each: the argument's rounding
is the same u |d| exp(-|d|), the result's at most 2 u of a value <= 1), adds three terms (2 roundings, relative, the sum
is >= 1: 2 u in the logarithm), takes __logf (v_log_f32 of one ulp and a product by ln 2, of a value <= log 3: 2.2 u):
at most 10 u whatever the magnitudes.  Then three roundings that ARE relative to the value: m + log, e + ., . - shift,
3 u V with V the magnitude of the shifted value.  The backward recurrence has the same count (B + e, the lse, the shift).
gamma(t, .) takes the forward chain over the frames up to t and the backward chain over those after t: (10 + 3 V) u per
frame, F frames.  Forming gamma: A + B, - top (2 u V), __expf (3 u), the sum of the row as one binary tree over the state
index (at most 10 levels of additions of non-negative terms: 10 u relative, gamma <= 1; 21 u is kept in the count), v_rcp_f32 and the product (2 u),
the 2^-30 fixed point (2^-31 per state, at most S <= 2 F + 1 states: below F u / 32): 27 u + 2 u V, once.  log_z takes the
forward chain, the float64 sum of the shifts (nothing at this scale) and ONE rounding to float32 of a value of
magnitude <= F E, E the largest |score|: u F E.
With V <= 10 and E <= 18 (the scores of these tests lie above -18; -inf rounds nothing):
    gamma, Gamma:  (10 + 30) F u + 47 u <= 64 F u for F >= 2, and for F = 1 there is no recurrence: 47 u <= 64 u
    log_z:         (10 + 30) F u + 18 F u = 58 F u <= 64 F u
V is the assumption in this: the shift keeps every row's maximum at 0, and a cell far below its row's maximum errs by
u |v| per rounding while it reaches a result through the weight exp(-|v|) of an lse -- unless it lies on the only way to
the end.  The tests print the measured maxima in units of F u; profiles/fullsum/README.md records them.
"""
import numpy as np
import pytest
import torch

import align_ref as ar
import fullsum_ref as fr
from test_convert_batch_gpu import _ragged, f32_models        # noqa: F401  (a fixture and its inputs; that file is not edited)

pytestmark = pytest.mark.gpu

K_BOUND = 64
U = 2.0 ** -24
FRAMES = (1, 2, 15, 16, 17, 33, 130)          # the seams of the prefetch depth and of the unrolling (4)
KINDS = ('logsoftmax', 'speech', 'neginf', 'flat')
FIELDS = ('log_z', 'class_post', 'state_post', 'occupancy')


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return np.ascontiguousarray(_np(t)).view(np.uint32)


def _log_softmax(x):
    x = x.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)


def _split(F, S, rng):
    """S positive durations that add up to F (F >= S)."""
    cuts = np.sort(rng.choice(np.arange(1, F), size=S - 1, replace=False)) if S > 1 else np.array([], int)
    return np.diff(np.concatenate([[0], cuts, [F]]))


def _scores(kind, F, C, seq, rng):
    """One utterance's scores [F, C]: log-softmax of noise; speech-like (a planted segmentation of the frames over the
    states of ``seq``, +5 on the true class's logit); log-softmax with -inf entries; flat."""
    if kind == 'flat':
        return np.full((F, C), -np.log(C), np.float32)
    x = rng.standard_normal((F, C)) * 2.0
    if kind == 'speech':
        x = x / 2.0
        S = len(seq)
        lab = np.repeat(np.clip(seq, 0, C - 1), _split(F, S, rng)) if F >= S else rng.randint(0, C, size=F)
        x[np.arange(F), lab] += 5.0
    x = _log_softmax(x)
    if kind == 'neginf':
        x[rng.rand(F, C) < 0.1] = -np.inf
    return x


def _batch(S, C, opt_mode, seed):
    """Every F of FRAMES x every kind, plus two utterances of S + 7 frames (so that the long sequences have feasible cases
    without optional states too): (score, seq, opt, n_frames, n_seq) with max_seq = S + 7.  Dense: where S > F every
    second state is optional, which makes the utterance feasible from F >= (S + 1) / 2 on; otherwise it is infeasible on
    purpose."""
    rng = np.random.RandomState(seed)
    cases = [(F, k) for F in FRAMES for k in KINDS] + [(S + 7, 'logsoftmax'), (S + 7, 'speech')]
    B, Fmax, Smax = len(cases), max(max(FRAMES), S + 7), S + 7
    score = rng.standard_normal((B, Fmax, C)).astype(np.float32)    # rows beyond n_frames are NOT neutral
    seq = rng.randint(0, C, size=(B, Smax)).astype(np.int32)        # (repeated classes throughout: C <= 256)
    opt = None
    if opt_mode == 'sparse':
        opt = (rng.rand(B, Smax) < 0.15).astype(np.uint8)
    elif opt_mode == 'dense':
        opt = (rng.rand(B, Smax) < 0.8).astype(np.uint8)
        for b, (F, _) in enumerate(cases):
            if S > F:
                opt[b, 1::2] = 1
    n_frames = np.array([F for F, _ in cases], np.int32)
    for b, (F, k) in enumerate(cases):
        score[b, :F] = _scores(k, F, C, seq[b, :S], rng)
    return score, seq, opt, n_frames, np.full((B,), S, np.int32)


def _compare(got, want, n_frames, what=''):
    """Every output against float64 within BOUND(F) of the utterance; exact zeros and -inf where there is no path.
    Returns (the number of feasible utterances, the largest error in units of F u)."""
    lz, cp, sp, occ = (_np(getattr(got, k)) for k in FIELDS)
    assert not np.isnan(lz).any() and not np.isnan(cp).any() and not np.isnan(sp).any() and not np.isnan(occ).any(), what
    assert np.array_equal(_np(got.feasible), np.isfinite(want.log_z)), what
    n, worst = 0, 0.0
    for b in range(len(lz)):
        F = int(n_frames[b])
        if not np.isfinite(want.log_z[b]):
            assert lz[b] == -np.inf and not cp[b].any() and not sp[b].any() and not occ[b].any(), (what, b)
            continue
        n += 1
        bound = K_BOUND * F * U
        errs = (abs(float(lz[b]) - want.log_z[b]), np.abs(cp[b] - want.class_post[b]).max(), np.abs(sp[b] - want.state_post[b]).max(),
                np.abs(occ[b] - want.occ[b]).max() / F)
        assert max(errs) <= bound, (what, b, F, errs, bound)
        worst = max(worst, max(errs) / (F * U))
    return n, worst


def _run(score, nf, seq, ns, opt, **kw):
    import evaluation as ev
    return ev.align_posterior_batch(score, nf, seq, ns, optional=opt, kind='log', return_states=True, **kw)


# ------------------------------------------------------------------------------------------------------------ (a) shapes
@pytest.mark.parametrize('C', [1, 61, 256])
@pytest.mark.parametrize('S', [1, 2, 63, 64, 65, 128, 129, 257])
def test_shapes_against_float64(S, C):
    """F over the prefetch and unrolling seams x S over the lane-ownership seams with max_seq = S + 7 (every K) x four
    kinds of scores x opt NULL / sparse / dense x C, repeated classes in every transcript."""
    n_feasible, n_none, worst = 0, 0, 0.0
    for opt_mode in ('none', 'sparse', 'dense'):
        score, seq, opt, nf, ns = _batch(S, C, opt_mode, seed=S * 7 + C)
        want = fr.fullsum_batch_f64(score, seq, opt, nf, ns)
        n, w = _compare(_run(score, nf, seq, ns, opt), want, nf, opt_mode)
        n_feasible, n_none, worst = n_feasible + n, n_none + len(nf) - n, max(worst, w)
    print('S = %d, C = %d: %d feasible, %d infeasible, largest error %.3f F u (bound %d F u)' % (S, C, n_feasible, n_none, worst, K_BOUND))
    assert n_feasible >= 6, n_feasible                               # (the long utterances at least)
    assert S < 3 or n_none >= 1


def test_the_longest_sequence_against_float64():
    """S = 1,024 (K = 16, the limit) at F = 1,100, speech-like, sparse optional states."""
    rng = np.random.RandomState(5)
    F, S, C = 1100, 1024, 61
    seq = rng.randint(0, C, size=(1, S)).astype(np.int32)
    opt = (rng.rand(1, S) < 0.15).astype(np.uint8)
    score = _scores('speech', F, C, seq[0], rng)[None]
    want = fr.fullsum_batch_f64(score, seq, opt, [F], [S])
    n, w = _compare(_run(score, [F], seq, [S], opt), want, [F])
    print('S = 1024, F = 1100: largest error %.3f F u (bound %d F u)' % (w, K_BOUND))
    assert n == 1


# ------------------------------------------------------------------------------------------------------- (b) exact cases
def _one_path(F, S, C, seed, repeat):
    """Scores 0 along one admissible path and -inf elsewhere; some states optional, some of those skipped by the path."""
    rng = np.random.RandomState(seed)
    opt = (rng.rand(S) < 0.3).astype(np.uint8)
    present = np.ones(S, bool)
    for s in range(S):                                              # a skipped state needs present neighbours
        if S > 1 and opt[s] and rng.rand() < 0.5 and (s == 0 or present[s - 1]):
            present[s] = False
    states = np.nonzero(present)[0]
    dur = _split(F, len(states), rng)
    path = np.repeat(states, dur)
    seq = (np.arange(S) % repeat if repeat else rng.permutation(C)[:S]).astype(np.int32)
    score = np.full((F, C), -np.inf, np.float32)
    score[np.arange(F), seq[path]] = 0.0
    occ = np.zeros(S)
    occ[states] = dur
    return score, seq, opt, path, occ


@pytest.mark.parametrize('F,S,C,repeat', [(1, 1, 1, 0), (9, 5, 256, 0), (130, 70, 256, 0), (100, 64, 7, 7), (400, 300, 11, 11), (1100, 1024, 61, 61)])
def test_one_path_is_exact(F, S, C, repeat):
    """log_z == 0.0, gamma exactly 0 or 1, class_post exactly one-hot, occ the integer durations, and the frame states
    gamma implies are align_batch's.  With ``repeat`` the classes recur every ``repeat`` states (several states of one
    class meet in Gamma; a state further than two away cannot be reached, so the path stays the only one)."""
    import evaluation as ev
    score, seq, opt, path, occ = _one_path(F, S, C, seed=F + S, repeat=repeat)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (d(score[None]), [F], d(seq[None]), [S])
    r = ev.align_posterior_batch(*args, optional=d(opt[None]), kind='log', return_states=True)
    assert float(r.log_z[0]) == 0.0 and bool(r.feasible[0])
    sp = _np(r.state_post)[0]
    want = np.zeros((F, S), np.float32)
    want[np.arange(F), path] = 1.0
    assert np.array_equal(sp, want)
    assert np.array_equal(_np(r.class_post)[0], np.where(np.isfinite(score), np.float32(1), np.float32(0)))
    assert np.array_equal(_np(r.occupancy)[0], occ.astype(np.float32))
    a = ev.align_batch(*args, optional=d(opt[None]), kind='log')
    assert np.array_equal(_np(a.frame_state)[0], sp.argmax(1)) and float(a.total[0]) == 0.0


# --------------------------------------------------------------------------------------------- (d) ragged, deterministic
def _ragged_case():
    rng = np.random.RandomState(11)
    Fmax, Smax, C = 140, 300, 61
    nf = np.array([140, 0, 33, 100, 17, 140, 1, 139, 64, 5], np.int32)
    ns = np.array([60, 10, 0, 300, 17, 129, 1, 65, 100, 9], np.int32)
    B = len(nf)
    seq = rng.randint(0, C, size=(B, Smax)).astype(np.int32)
    seq[0, 3] = 61                                                   # an out-of-range class on the device: -inf
    seq[5, 7] = -5
    opt = (rng.rand(B, Smax) < 0.3).astype(np.uint8)
    opt[0, 3] = opt[5, 7] = 1                                        # (optional: the utterances stay feasible)
    opt[8, 1::2] = 1                                                 # 100 states in 64 frames
    score = rng.standard_normal((B, Fmax, C)).astype(np.float32)
    for b in range(B):
        if nf[b]:
            score[b, :nf[b]] = _scores(KINDS[b % 2], int(nf[b]), C, seq[b, :max(ns[b], 1)], rng)
    score[7, 70, :] = -np.inf                                        # a frame whose every state is -inf: no path
    return score, seq, opt, nf, ns


def test_ragged_batch_alone_twice_inputs_and_fills():
    """Feasible, infeasible and zero-length utterances and out-of-range classes in one batch, outputs on NaN-poisoned
    memory: within the bound of float64, zeros from F / S on, no NaN; each utterance alone (its own tight shapes: another
    K, another workspace) gives the same bits; two runs are bit-identical; the inputs are untouched."""
    from conftest import poison_gpu_state
    score, seq, opt, nf, ns = _ragged_case()
    B = len(nf)
    want = fr.fullsum_batch_f64(score, seq, opt, nf, ns)
    feas = np.isfinite(want.log_z)
    assert feas.sum() >= 5 and feas[0] and feas[5] and feas[8] and not feas[1] and not feas[2] and not feas[3] and not feas[7], feas
    d_score, d_seq, d_opt = (torch.from_numpy(v).cuda() for v in (score, seq, opt))
    d_nf, d_ns = torch.from_numpy(nf).cuda(), torch.from_numpy(ns).cuda()
    poison_gpu_state()
    got = _run(d_score, d_nf, d_seq, d_ns, d_opt)
    n, w = _compare(got, want, nf)
    print('ragged: %d feasible, largest error %.3f F u' % (n, w))
    for b in range(B):                                              # the fills, spelled out
        F, S = (int(nf[b]), int(ns[b])) if feas[b] else (0, 0)
        assert not _np(got.class_post)[b, F:].any() and not _np(got.state_post)[b, F:].any()
        assert not _np(got.state_post)[b, :, S:].any() and not _np(got.occupancy)[b, S:].any()
    poison_gpu_state()
    again = _run(d_score, d_nf, d_seq, d_ns, d_opt)
    for k in FIELDS:
        assert np.array_equal(_bits(getattr(got, k)), _bits(getattr(again, k))), k
    assert np.array_equal(_np(d_score).view(np.uint32), score.view(np.uint32)) and np.array_equal(_np(d_seq), seq)
    assert np.array_equal(_np(d_opt), opt) and np.array_equal(_np(d_nf), nf) and np.array_equal(_np(d_ns), ns)
    import evaluation as ev
    no_states = ev.align_posterior_batch(d_score, d_nf, d_seq, d_ns, optional=d_opt, kind='log')
    assert no_states.state_post is None
    for k in ('log_z', 'class_post', 'occupancy'):
        assert np.array_equal(_bits(getattr(got, k)), _bits(getattr(no_states, k))), k
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # (device arrays: seq is not range-checked)
    for b in (0, 3, 4, 5, 6, 7, 8, 9):
        F, S = int(nf[b]), int(ns[b])
        one = _run(dev(score[b:b + 1, :F]), [F], dev(seq[b:b + 1, :S]), [S], dev(opt[b:b + 1, :S]))
        assert _bits(one.log_z)[0] == _bits(got.log_z)[b], b
        assert np.array_equal(_bits(one.class_post)[0], _bits(got.class_post)[b, :F]), b
        assert np.array_equal(_bits(one.state_post)[0], _bits(got.state_post)[b, :F, :S]), b
        assert np.array_equal(_bits(one.occupancy)[0], _bits(got.occupancy)[b, :S]), b


def test_graph_replay_with_new_contents_and_lengths():
    """The two launches captured on static buffers with the lengths in device tensors, replayed after other contents and
    other lengths were copied into the same buffers: the bits of the eager public call.  The first call is outside the
    capture."""
    import evaluation as ev
    rng = np.random.RandomState(41)
    B, F, S, C = 5, 70, 130, 61

    def contents(nf, ns):
        seq = rng.randint(0, C, size=(B, S)).astype(np.int32)
        opt = (rng.rand(B, S) < 0.3).astype(np.uint8)
        opt[:, 1::2] |= np.array(ns)[:, None] > np.array(nf)[:, None]
        score = rng.standard_normal((B, F, C)).astype(np.float32)
        for b in range(B):
            if nf[b]:
                score[b, :nf[b]] = _scores(KINDS[b % 4], nf[b], C, seq[b, :max(ns[b], 1)], rng)
        return score, seq, opt

    nf0, ns0 = [70, 33, 16, 64, 1], [20, 33, 5, 130, 1]
    h = contents(nf0, ns0)
    d_score, d_seq, d_opt = (torch.from_numpy(v).cuda() for v in h)
    d_nf, d_ns = torch.tensor(nf0, dtype=torch.int32, device='cuda'), torch.tensor(ns0, dtype=torch.int32, device='cuda')
    ev._fullsum_launch(d_score, d_seq, d_opt, d_nf, d_ns, True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = ev._fullsum_launch(d_score, d_seq, d_opt, d_nf, d_ns, True)

    def check(h, nf, ns):
        g.replay()
        torch.cuda.synchronize()
        eager = _run(h[0], nf, h[1], ns, h[2])
        want = fr.fullsum_batch_f64(h[0], h[1], h[2], nf, ns)
        n, _ = _compare(out, want, nf)
        for k in FIELDS:
            assert np.array_equal(_bits(getattr(out, k)), _bits(getattr(eager, k))), k
        return n, _np(out.class_post).copy()

    n0, c0 = check(h, nf0, ns0)
    assert n0 >= 3
    nf1, ns1 = [17, 70, 0, 2, 69], [17, 65, 9, 2, 30]
    h1 = contents(nf1, ns1)
    for d, v in zip((d_score, d_seq, d_opt), h1):
        d.copy_(torch.from_numpy(v))
    d_nf.copy_(torch.tensor(nf1, dtype=torch.int32))
    d_ns.copy_(torch.tensor(ns1, dtype=torch.int32))
    n1, c1 = check(h1, nf1, ns1)
    assert n1 >= 3 and not np.array_equal(c0, c1)


# ------------------------------------------------------------------------------------------------------ (e) loud dead end
def test_loud_mass_in_a_dead_end_stays_feasible():
    """F = 40, S = 8, nothing optional; state 0 scores 0 on every frame, every other state log(1e-10): nearly all of the
    forward mass sits in state 0, which cannot reach the end after frame 32 -- a scaled linear recurrence normalises by that
    mass and loses the paths that do arrive; the shifted log domain keeps them."""
    F, S = 40, 8
    score = np.full((1, F, S), np.log(1e-10), np.float32)
    score[0, :, 0] = 0.0
    seq = np.arange(S, dtype=np.int32)[None]
    want = fr.fullsum_batch_f64(score, seq, None, [F], [S])
    assert np.isfinite(want.log_z[0]) and want.log_z[0] < -150.0
    got = _run(score, [F], seq, [S], None)
    n, w = _compare(got, want, [F])
    print('loud dead end: log_z %.6f (float64 %.6f), largest error %.3f F u' % (float(got.log_z[0]), want.log_z[0], w))
    assert n == 1 and bool(got.feasible[0])


# ------------------------------------------------------------------------------------------------------- the public calls
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


def test_public_calls_kinds_and_no_synchronisation(wav_case):
    """kind='prob' (floored), 'log' and 'logits' against the reference fed with the scores each kind defines;
    align_posterior_wav_batch against align_posterior_batch on content_wav_batch's posteriors; all under
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
    logits = (rng.standard_normal((B, F, C)) * 2.0).astype(np.float32)
    nf, ns = [36, 70, 50, 1], [12, 12, 9, 1]
    seq = rng.randint(0, C, size=(B, S)).astype(np.int32)
    opt = (rng.rand(B, S) < 0.3).astype(np.uint8)
    d_ppg, d_logits, d_wav = torch.from_numpy(ppg).cuda(), torch.from_numpy(logits).cuda(), torch.from_numpy(w['wav']).cuda()
    calls = (lambda: ev.align_posterior_batch(d_ppg, nf, seq, ns, optional=opt, kind='prob', floor=1e-6, return_states=True),
             lambda: ev.align_posterior_batch(d_logits, nf, seq, ns, optional=opt, kind='logits', return_states=True),
             lambda: ev.align_posterior_wav_batch(w['enc'], d_wav, w['lens'], w['seq'], w['n_seq'], w['c'], return_states=True),
             lambda: ev.align_posterior_wav_batch(w['enc'], d_wav, w['lens'], w['seq'], w['n_seq'], w['c'], ppg=w['ppg']))
    for c in calls:
        c()
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        a, lg, wv, wp = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    logged = _np(torch.log(d_ppg.clamp_min(1e-6)))
    assert np.isfinite(logged).all() and logged[0, 5, 0] < -13.0                  # the floor was applied
    n, _ = _compare(a, fr.fullsum_batch_f64(logged, seq, opt, nf, ns), nf)
    n2, _ = _compare(lg, fr.fullsum_batch_f64(_np(torch.log_softmax(d_logits, -1)), seq, opt, nf, ns), nf)
    assert n >= 3 and n2 >= 3
    # waveforms in
    assert torch.equal(wv.ppg, w['ppg']) and torch.equal(wv.n_frames, w['n_frames']) and wp.state_post is None
    want = ev.align_posterior_batch(w['ppg'], w['n_frames'], w['seq'], w['n_seq'], return_states=True)
    assert bool(want.feasible.all())                                 # the transcript came from these posteriors
    for k in FIELDS:
        assert np.array_equal(_bits(getattr(wv, k)), _bits(getattr(want, k))), k
    for k in ('log_z', 'class_post', 'occupancy'):
        assert np.array_equal(_bits(getattr(wp, k)), _bits(getattr(want, k))), k
    # the full sum is at least the best path; the expected durations add up to the frame counts
    best = ev.align_batch(w['ppg'], w['n_frames'], w['seq'], w['n_seq'])
    assert bool((want.log_z >= best.total - 1e-3).all())
    assert np.abs(_np(want.occupancy).sum(1) - _np(w['n_frames'])).max() < 1e-2


def test_limits_raise_value_error():
    import evaluation as ev
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='1024'):
        ev.align_posterior_batch(z(1, 4, 3), [4], zi(1, 1025), [2])
    with pytest.raises(ValueError, match='4096'):
        ev.align_posterior_batch(z(1, 1, 4097), [1], zi(1, 1), [1])
    with pytest.raises(ValueError, match='2 GiB'):
        ev.align_posterior_batch(np.broadcast_to(np.float32(0), (256, 2048, 1)), [1] * 256, zi(256, 1024), [1] * 256)
    r = ev.align_posterior_batch(z(1, 4, 4096), [4], zi(1, 1024), [2], kind='log', return_states=True)      # at the limits: runs
    assert abs(float(r.log_z[0]) - np.log(3.0)) <= K_BOUND * 4 * U   # three paths of score 0
    assert abs(float(r.class_post[0, :, 0].sum()) - 4.0) <= 1e-5 and not bool(r.class_post[0, :, 1:].any())


# ------------------------------------------------------------------------------------------------------------ (f) trainer
def _encoder(golden_dir):
    import json
    import os
    from conftest import ROOT
    from encoder import encoder_spec_phn
    cfg = json.load(open(os.path.join(ROOT, 'speech-cloner_amd', 'hp', 'encoder_cfg_d.json')))
    cfg.update(is_training=True, model_path=os.path.join(golden_dir, 'enc_14_ckpt'), dropout_seed=5)
    enc = encoder_spec_phn(cfg, None)
    enc.restore()
    return enc, enc._get_trainer()


def _encoder_input(golden_dir, N):
    import os
    g = np.load(os.path.join(golden_dir, 'encoder_fwd.npz'))
    return np.stack([np.roll(g['x'][i % 3], 16 * (3 + 5 * i), axis=0) for i in range(N)]).astype(np.float32)


def test_trainer_gradient_is_softmax_minus_gamma(golden_dir):
    """The shipped encoder configuration at 2 windows (the smallest the existing encoder training test uses), ragged: the
    gradient at the logits against (softmax(y) - Gamma64) / M, Gamma64 from the restatement on the downloaded logits.
    Bound: BOUND(F) / M for Gamma, plus the rounding of vc_softmax_ce's own (softmax sum(target) - target) / M -- the
    row's exponentials (2 u), their sum over 61 classes (61 u at worst), the quotient (u), the sum of the target row (64 u;
    the row of Gamma adds up to 1 within the 24 u of gamma's normalisation) and the two products (2 u): below 160 u / M for
    a value <= 1.  Exactly zero on padded frames: their target rows are zero."""
    enc, tr = _encoder(golden_dir)
    N, T, C = 2, 400, 61
    x = _encoder_input(golden_dir, N)
    nf = np.array([400, 250], np.int32)
    x[1, 250:] = 0.0
    rng = np.random.RandomState(7)
    S = 60
    seq = rng.randint(0, C, size=(N, S)).astype(np.int32)
    opt = (rng.rand(N, S) < 0.2).astype(np.uint8)
    ns = np.array([60, 41], np.int32)
    out3, log_z = tr.forward_backward_transcript(torch.from_numpy(x).cuda(), nf, seq, ns, optional=opt)
    torch.cuda.synchronize()
    M = N * T
    y = _np(tr.y_logits)[:, :C].astype(np.float64).reshape(N, T, C)
    dy = _np(tr.dy_logits)
    assert not dy[:, C:].any()
    dy = dy[:, :C].reshape(N, T, C)
    ls = y - y.max(-1, keepdims=True)
    ls = ls - np.log(np.exp(ls).sum(-1, keepdims=True))
    want = fr.fullsum_batch_f64(ls, seq, opt, nf, ns)
    assert np.isfinite(want.log_z).all()
    for b in range(N):
        F = int(nf[b])
        bound = (K_BOUND * F * U + 160 * U) / M
        err = np.abs(dy[b, :F] - (np.exp(ls[b, :F]) - want.class_post[b, :F]) / M).max()
        lz_err = abs(float(log_z[b]) - want.log_z[b])
        print('trainer utterance %d: gradient error %.3e (bound %.3e), log_z error %.3f F u' % (b, err, bound, lz_err / (F * U)))
        assert err <= bound and lz_err <= K_BOUND * F * U
        assert not dy[b, F:].any()                                  # exactly zero on padded frames
    assert np.isfinite(_np(out3)).all()
    assert float(tr.grad.abs().max()) > 0.0


def test_trainer_one_path_equals_the_one_hot_step_bit_for_bit(golden_dir):
    """F == S == T for every utterance, nothing optional, no padding: the diagonal is the only path, Gamma is exactly
    one-hot, and out3 and the flat gradient buffer equal those of a second, identically built and seeded trainer's
    forward_backward(x, onehot)."""
    N, T, C = 2, 400, 61
    x = torch.from_numpy(_encoder_input(golden_dir, N)).cuda()
    labels = np.random.RandomState(9).randint(0, C, size=(N, T)).astype(np.int32)
    onehot = torch.from_numpy(np.eye(C, dtype=np.float32)[labels]).cuda()
    enc_a, tr_a = _encoder(golden_dir)
    out_a, log_z = tr_a.forward_backward_transcript(x, [T] * N, labels, [T] * N)
    enc_b, tr_b = _encoder(golden_dir)
    out_b = tr_b.forward_backward(x, onehot)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(tr_a.y_logits), _bits(tr_b.y_logits))
    assert np.array_equal(_bits(out_a), _bits(out_b)), (_np(out_a), _np(out_b))
    assert np.array_equal(_bits(tr_a.grad), _bits(tr_b.grad))
    assert float(tr_a.grad.abs().max()) > 0.0
    # log Z of the one path is the sum of its log-posteriors: the cross-entropy total with the sign turned
    assert abs(float(log_z.sum()) + float(out_a[0]) * N * T) <= 1e-4 * abs(float(log_z.sum()))
