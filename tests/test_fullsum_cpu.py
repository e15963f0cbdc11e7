"""Full-sum alignment without a GPU: the float64 restatement tests/fullsum_ref.py against brute force, against forced
alignment, against autograd; the exports and the argument checks that come before any GPU use."""
import itertools
import os
import re

import numpy as np
import pytest

import align_ref as ar
import fullsum_ref as fr
from conftest import ROOT


def _scores(rng, F, C, p_inf=0.15):
    x = rng.standard_normal((F, C)) * 2.0
    x[rng.rand(F, C) < p_inf] = -np.inf
    return x


def test_reference_equals_brute_force():
    """Every F <= 6, S <= 4 and every opt pattern, scores with -inf among them: log Z and gamma of the recurrences against
    the enumeration of every admissible path, to 1e-12; no path: -inf and zeros on both sides."""
    rng = np.random.RandomState(0)
    n_feasible = n_none = 0
    for F, S in itertools.product(range(1, 7), range(1, 5)):
        for opt in itertools.product((0, 1), repeat=S):
            C = 3
            score, seq = _scores(rng, F, C, p_inf=0.08), rng.randint(0, C, size=S)
            lz, g = fr.brute_force(score, seq, opt)
            r = fr.fullsum_f64(score, seq, opt)
            if lz == -np.inf:
                n_none += 1
                assert r.log_z == -np.inf and not r.state_post.any() and not r.class_post.any() and not r.occ.any()
                continue
            n_feasible += 1
            assert abs(r.log_z - lz) <= 1e-12 * max(1.0, abs(lz)), (F, S, opt)
            assert np.abs(r.state_post - g).max() <= 1e-12, (F, S, opt)
            want = np.zeros((F, C))
            for s in range(S):
                want[:, seq[s]] += g[:, s]
            assert np.abs(r.class_post - want).max() <= 1e-12 and np.abs(r.occ - g.sum(0)).max() <= 1e-12
    assert n_feasible >= 100 and n_none >= 30, (n_feasible, n_none)


def test_log_z_bounds_the_best_path_and_equals_it_when_there_is_one_path():
    rng = np.random.RandomState(1)
    for F, S in ((9, 4), (12, 12), (7, 3), (20, 11)):
        C = 5
        score, seq = _scores(rng, F, C, p_inf=0.05), rng.randint(0, C, size=S)
        opt = (rng.rand(S) < 0.3).astype(np.uint8) if F > S else None
        best = ar.align_f64(score, seq, opt)
        r = fr.fullsum_f64(score, seq, opt)
        assert r.log_z >= best.total - 1e-12 * max(1.0, abs(best.total))
        if F == S and np.isfinite(best.total):                      # the diagonal is the only path
            assert abs(r.log_z - best.total) <= 1e-12 * abs(best.total)
            assert np.array_equal(r.state_post, np.eye(F))
    # one path by construction: 0 along it, -inf elsewhere
    seq, dur = np.arange(6), [2, 1, 3, 1, 1, 2]
    score = np.full((10, 6), -np.inf)
    score[np.arange(10), np.repeat(seq, dur)] = 0.0
    r = fr.fullsum_f64(score, seq)
    assert r.log_z == 0.0 == ar.align_f64(score, seq).total and r.occ.tolist() == dur
    assert np.array_equal(r.class_post, np.where(np.isfinite(score), 1.0, 0.0))


def test_every_feasible_row_of_gamma_sums_to_one():
    rng = np.random.RandomState(2)
    n = 0
    for F, S, C in ((1, 1, 1), (30, 7, 4), (40, 40, 9), (130, 65, 61), (33, 50, 5)):
        seq = rng.randint(0, C, size=S)
        opt = (rng.rand(S) < (0.9 if S > F else 0.2)).astype(np.uint8)
        if S > F:
            opt[1::2] = 1
        r = fr.fullsum_f64(_scores(rng, F, C, p_inf=0.02), seq, opt)
        if r.log_z == -np.inf:
            continue
        n += 1
        assert np.abs(r.state_post.sum(1) - 1.0).max() <= 1e-12 and np.abs(r.class_post.sum(1) - 1.0).max() <= 1e-12
        assert abs(r.occ.sum() - F) <= 1e-12 * F
    assert n >= 4


def test_softmax_minus_class_post_is_the_gradient_of_minus_log_z():
    """float64 autograd through the recurrences written with torch.logsumexp on log_softmax(y); -1e30 stands in for -inf in
    the graph (logsumexp of nothing but -inf has a NaN gradient)."""
    import torch
    rng = np.random.RandomState(3)
    F, S, C = 11, 5, 4
    seq = np.array([2, 0, 3, 0, 1])
    opt = np.array([0, 1, 0, 1, 0], np.uint8)
    y = torch.tensor(rng.standard_normal((F, C)) * 2.0, dtype=torch.float64, requires_grad=True)
    e = torch.log_softmax(y, dim=-1)[:, torch.from_numpy(seq)]
    big = torch.tensor(-1e30, dtype=torch.float64)
    la = [torch.stack([e[0, s] if s == 0 or (s == 1 and opt[0]) else big for s in range(S)])]
    for t in range(1, F):
        p, row = la[-1], []
        for s in range(S):
            terms = [p[s]] + ([p[s - 1]] if s >= 1 else []) + ([p[s - 2]] if s >= 2 and opt[s - 1] else [])
            row.append(e[t, s] + torch.logsumexp(torch.stack(terms), 0))
        la.append(torch.stack(row))
    ends = [la[-1][S - 1]] + ([la[-1][S - 2]] if opt[S - 1] else [])
    log_z = torch.logsumexp(torch.stack(ends), 0)
    (-log_z).backward()
    r = fr.fullsum_f64(torch.log_softmax(y, -1).detach().numpy(), seq, opt)
    assert abs(float(log_z.detach()) - r.log_z) <= 1e-12 * abs(r.log_z)
    want = torch.softmax(y, -1).detach().numpy() - r.class_post
    assert np.abs(y.grad.numpy() - want).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------- exports
def test_exports_workspace_query_and_c_argument_checks():
    import ctypes
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    lib = _vc.lib()
    for name in ('vc_fullsum_workspace_bytes', 'vc_fullsum_f32'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _vc._SIGS and hasattr(lib, name)
    q = lib.vc_fullsum_workspace_bytes
    a256 = lambda v: (v + 255) // 256 * 256
    assert q(16, 1000, 300) == a256(16 * 1000 * 300 * 4) and q(3, 7, 5) == a256(3 * 7 * 5 * 4) and q(1, 1, 1) == 256
    assert q(0, 10, 10) == 0 and q(65536, 10, 10) == 0 and q(1, 10, 1025) == 0 and q(1, 10, 0) == 0 and q(1, 0, 10) == 0
    assert q(1, 2 ** 29 - 64, 1) > 0 and q(1, 2 ** 29, 1) == 0 and q(256, 2048, 1024) == 0 and q(256, 2047, 1024) > 0     # 2 GiB
    f = lib.vc_fullsum_f32
    p = ctypes.c_void_p(4096)
    ok = dict(score=p, seq=p, opt=None, nf=p, ns=p, B=1, F=10, S=10, C=61, lz=p, cp=p, sp=None, occ=p, ws=p, wb=1 << 20, stream=None)
    call = lambda **kw: f(*dict(ok, **kw).values())
    for k in ('score', 'seq', 'nf', 'ns', 'lz', 'cp', 'occ', 'ws'):
        assert call(**{k: None}) == 1 and b'vc_fullsum_f32: NULL' in lib.vc_last_error(), k
    for kw in (dict(B=0), dict(F=0), dict(S=0), dict(C=0)):
        assert call(**kw) == 1 and b'vc_fullsum_f32: bad shape' in lib.vc_last_error(), kw
    for kw in (dict(B=65536), dict(S=1025), dict(C=4097), dict(B=256, F=2048, S=1024)):
        assert call(**kw) == 4 and b'vc_fullsum_f32: limits' in lib.vc_last_error(), kw
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
    monkeypatch.setattr(ev, '_fullsum_launch', no_gpu)
    B, F, C, S = 2, 20, 61, 5
    ppg = np.full((B, F, C), 1.0 / C, np.float32)
    seq = np.zeros((B, S), np.int32)
    good = dict(ppg=ppg, lens=[20, 10], seq=seq, n_seq=[5, 3])
    bad = [dict(ppg=ppg[0]), dict(ppg=ppg.astype(np.float64)), dict(ppg=np.broadcast_to(np.float32(0), (B, F, 4097))),
           dict(lens=[20]), dict(lens=[21, 1]), dict(lens=[-1, 1]), dict(lens=[1.5, 2.0]),
           dict(seq=seq[0]), dict(seq=seq.astype(np.int64)), dict(seq=np.zeros((3, S), np.int32)), dict(seq=np.zeros((B, 1025), np.int32)),
           dict(seq=np.full((B, S), 61, np.int32)), dict(seq=np.full((B, S), -1, np.int32)),
           dict(n_seq=[6, 1]), dict(n_seq=[1]), dict(n_seq=[-1, 1]),
           dict(optional=np.zeros((B, S + 1), np.uint8)), dict(optional=np.zeros((B, S), np.int32)),
           dict(kind='logit'), dict(floor=0.0), dict(floor=float('nan')), dict(floor=-1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            ev.align_posterior_batch(**dict(good, **kw))
    for kind in ('prob', 'log', 'logits'):                          # all three kinds pass the checks
        with pytest.raises(AssertionError, match='touched'):
            ev.align_posterior_batch(**dict(good, kind=kind))
    with pytest.raises(ValueError, match="'prob', 'log' or 'logits'"):
        ev.align_posterior_batch(**dict(good, kind='posterior'))
    with pytest.raises(ValueError, match="'prob' or 'log'"):        # (forced alignment takes no logits)
        ev.align_batch(**dict(good, kind='logits'))
    with pytest.raises(ValueError, match='2 GiB'):
        ev.align_posterior_batch(np.broadcast_to(np.float32(0), (256, 2048, 1)), [1] * 256, np.zeros((256, 1024), np.int32), [1] * 256)
    # align_posterior_wav_batch
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
            ev.align_posterior_wav_batch(**dict(gw, **kw))

    class Wide:
        cfg_d = {'n_output': 4097}
    with pytest.raises(ValueError, match='4096'):
        ev.align_posterior_wav_batch(**dict(gw, encoder=Wide()))
    with pytest.raises(AssertionError, match='touched'):
        ev.align_posterior_wav_batch(**gw)
    monkeypatch.undo()
    if not torch.cuda.is_available():
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            ev.align_posterior_batch(**good)


def test_trainer_argument_errors_come_before_any_launch():
    """forward_backward_transcript checks n_frames, seq, n_seq and optional before it touches the trainer or the GPU."""
    import training

    class Fake:
        cfg = {'n_output': 61}

        def _drain_pending(self):
            raise AssertionError('the trainer was touched before the argument check')
    x = np.zeros((2, 40, 80), np.float32)
    seq = np.zeros((2, 5), np.int32)
    call = lambda **kw: training.EncoderTrainer.forward_backward_transcript(Fake(), **dict(dict(x=x, n_frames=[40, 30], seq=seq, n_seq=[5, 3]), **kw))
    for kw in (dict(n_frames=[41, 1]), dict(n_frames=[40]), dict(seq=np.full((2, 5), 61, np.int32)), dict(seq=seq.astype(np.int64)),
               dict(n_seq=[6, 1]), dict(optional=np.zeros((2, 6), np.uint8)), dict(seq=np.zeros((2, 1025), np.int32))):
        with pytest.raises(ValueError):
            call(**kw)
