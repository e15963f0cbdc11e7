"""The content scores without a GPU: tests/content_ref.py against hand-worked cases, the class tables, the exported
symbols and every host-side refusal of the new calls in evaluation.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import content_ref as cr
from conftest import ROOT


def _onehot(labels, C):
    x = np.zeros((len(labels), C), np.float32)
    x[np.arange(len(labels)), labels] = 1.0
    return x


# ------------------------------------------------------------------------------------------------ the reference itself
def test_edit_distance_tie_order_on_a_two_symbol_alphabet():
    """a = [0, 1], b = [1, 0].  E(1, 1) = 1 by the diagonal (a substitution); at (1, 2) the diagonal from E(0, 1) = 1 with a
    match gives 1 and wins outright; at (2, 1) likewise; at (2, 2) the diagonal gives E(1, 1) + 1 = 2, up gives
    E(1, 2) + 1 = 2, left gives E(2, 1) + 1 = 2: all three tie, and the diagonal is taken -- two substitutions, not a
    deletion and an insertion around a match."""
    r = cr.edit_distance([0, 1], [1, 0])
    assert (r['dist'], r['n_match'], r['n_sub'], r['n_del'], r['n_ins']) == (2, 0, 2, 0, 0) and r['per'] == 1.0
    # up before left: a = [0, 0], b = [0]: at (2, 1) the diagonal costs E(1, 0) + 0 = 1, up E(1, 1) + 1 = 1: the diagonal
    # wins the tie, so the match is a's SECOND symbol and the first one is the deletion (via column 0)
    r = cr.edit_distance([0, 0], [0])
    assert (r['dist'], r['n_match'], r['n_sub'], r['n_del'], r['n_ins']) == (1, 1, 0, 1, 0)
    r = cr.edit_distance([0], [0, 0])
    assert (r['dist'], r['n_match'], r['n_sub'], r['n_del'], r['n_ins']) == (1, 1, 0, 0, 1)
    # the empty sides
    assert cr.edit_distance([], [3, 4])['n_ins'] == 2 and np.isnan(cr.edit_distance([], [3, 4])['per'])
    r = cr.edit_distance([3, 4, 5], [])
    assert (r['dist'], r['n_del'], r['per']) == (3, 3, 1.0)
    r = cr.edit_distance([1, 2, 3, 4], [1, 3, 9])                  # one deletion (2), one substitution (4 -> 9)
    assert (r['dist'], r['n_match'], r['n_sub'], r['n_del'], r['n_ins'], r['per']) == (2, 2, 1, 1, 0, 0.5)


def test_segments_drop_after_merge_and_short_runs():
    a, x, pau = 0, 1, 2
    cmap = np.array([0, 1, -1], np.int32)
    # a pau a: the pause is long enough to survive, separates the two a, and is then dropped: two segments
    lab, st, en = cr.phn_segments(_onehot([a] * 4 + [pau] * 3 + [a] * 5, 3), 12, cmap, min_run=3)
    assert (lab, st, en) == ([a, a], [0, 7], [4, 12])
    # a x a with a short x: x leaves in step 3, the two a are neighbours in step 4 and merge over it
    lab, st, en = cr.phn_segments(_onehot([a] * 4 + [x] * 2 + [a] * 5, 3), 11, cmap, min_run=3)
    assert (lab, st, en) == ([a], [0], [11])
    # not iterated: a short pause between two a merges them too (the pause never became a segment)
    lab, st, en = cr.phn_segments(_onehot([a] * 4 + [pau] * 2 + [a] * 5, 3), 11, cmap, min_run=3)
    assert (lab, st, en) == ([a], [0], [11])
    # min_run > F: nothing survives; F = 0: nothing to begin with
    assert cr.phn_segments(_onehot([a] * 5, 3), 5, None, min_run=6) == ([], [], [])
    assert cr.phn_segments(_onehot([a] * 5, 3), 0, None, min_run=1) == ([], [], [])
    # the lowest index wins an arg-max tie
    assert cr.frame_labels(np.array([[0.25, 0.5, 0.5], [0.5, 0.5, 0.0]], np.float32), 2) == [1, 0]
    l, s, e, n = cr.padded_segments(_onehot([a] * 3 + [x] * 3, 3), 6, 8, None, 3)
    assert n == 2 and l.tolist() == [0, 1] + [-1] * 6 and s.tolist() == [0, 3] + [-1] * 6 and e.tolist() == [3, 6] + [-1] * 6


def test_js_of_disjoint_one_hots_is_one_bit_and_of_equal_rows_zero():
    p, q = _onehot([0], 4)[0], _onehot([3], 4)[0]
    assert cr.js_bits(p, q) == 1.0 and cr.js_bits(p, p) == 0.0
    u = np.full(4, 0.25, np.float32)
    assert cr.js_bits(u, u) == 0.0
    # p = (1/2, 1/2, 0, 0), q = (0, 1/2, 1/2, 0): m = (1/4, 1/2, 1/4, 0); 0.5 * (1/2 + 0 + 0 + 1/2) = 0.5 bit
    assert cr.js_bits(np.array([0.5, 0.5, 0, 0]), np.array([0, 0.5, 0.5, 0])) == 0.5
    a = np.stack([p, q, p]).astype(np.float32)
    # cells (p, q): 1 bit, labels 0 and 3; (q, q): 0; (p, u): m = (5/8, 1/8, 1/8, 1/8), labels 0 and 0 (the lowest index)
    js_pu = 0.5 * (np.log2(1.6) + 0.25 * np.log2(0.4) + 0.75)
    r = cr.ppg_metrics(a, np.stack([q, q, u]), 3, 3)
    assert (r['n_cells'], r['n_agree']) == (3, 2) and r['js_mean'] == pytest.approx((1.0 + js_pu) / 3.0, abs=1e-15)
    r = cr.ppg_metrics(a, a, 3, 3, path=np.array([[0, 0], [1, 1], [5, 0], [-1, -1]]))
    assert (r['n_cells'], r['n_agree'], r['frame_agreement'], r['js_mean']) == (2, 2, 1.0, 0.0)
    assert np.isnan(cr.ppg_metrics(a, a, 3, 3, path=np.array([[-1, -1]]))['js_mean'])


# ------------------------------------------------------------------------------------------------------- the class tables
def test_class_map_and_the_39_fold():
    import evaluation as ev
    import sound_ds
    names = sound_ds.TIMIT_PHONEMES_61
    t = ev.class_map(names)
    assert t.dtype == np.int32 and t.shape == (61,)
    assert len(set(t[t >= 0].tolist())) == 39
    for n, rep in ev.TIMIT_FOLD_39.items():
        if n in ('pau', 'epi', 'h#'):
            continue
        assert t[names.index(n)] == (-1 if rep is None else names.index(rep)), n
    for n in ('pau', 'epi', 'h#', 'q'):
        assert t[names.index(n)] == -1, n
    for n in names:                                                 # a representative stands for itself
        if n not in ev.TIMIT_FOLD_39 and n not in ('pau', 'epi', 'h#'):
            assert t[names.index(n)] == names.index(n), n
    assert set(ev.TIMIT_FOLD_39.values()) - {None} <= set(names) and set(ev.TIMIT_FOLD_39) <= set(names)
    ident = ev.class_map(names, fold=None, drop=())
    assert ident.tolist() == list(range(61))
    arc = sound_ds.ARCTIC_PHONEMES_43
    ta = ev.class_map(arc, drop=('pau', 'H#', 'ssil'))
    assert ta[arc.index('ax')] == arc.index('ah') and ta[arc.index('ao')] == arc.index('aa') and ta[arc.index('zh')] == arc.index('sh')
    assert [ta[arc.index(n)] for n in ('pau', 'H#', 'ssil')] == [-1, -1, -1] and ta.min() == -1 and ta.max() < 43
    with pytest.raises(ValueError):
        ev.class_map([])
    with pytest.raises(ValueError):
        ev.class_map(['a', 'a'])
    with pytest.raises(ValueError):
        ev.class_map(['c%d' % i for i in range(257)])


# ------------------------------------------------------------------------------------------------------- ABI and refusals
NEW = ('vc_ppg_metrics_f32', 'vc_phn_segments_tile', 'vc_phn_segments', 'vc_edit_distance_rows', 'vc_edit_distance_workspace_bytes',
       'vc_edit_distance_i32')


def test_exports_constants_and_refusals_before_any_hip_call():
    import _vc
    import evaluation as ev
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _vc.lib()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _vc._SIGS and hasattr(lib, name), name
    assert lib.vc_version() == _vc.VC_ABI_VERSION                   # added without a version bump
    assert os.path.exists(os.path.join(ROOT, 'speech-cloner_amd', 'csrc', 'vc_content.hip'))
    assert lib.vc_phn_segments_tile() == ev.SEGMENT_TILE and lib.vc_edit_distance_rows() == ev.EDIT_ROWS
    assert lib.vc_edit_distance_workspace_bytes(3, 100, 50) == ((3 * 2 * 50 * 16 + 255) // 256) * 256
    assert lib.vc_edit_distance_workspace_bytes(1, 16384, 16385) == 0 and lib.vc_edit_distance_workspace_bytes(65536, 8, 8) == 0
    p = ctypes.c_void_p(4096)                                       # non-NULL, aligned, never dereferenced
    INVALID, WORKSPACE, UNSUPPORTED = 1, 3, 4                     # VC_ERR_* of include/vc_hip.h
    assert lib.vc_ppg_metrics_f32(None, p, p, p, 1, 4, 4, 61, None, None, 0, None, p, p, None) == INVALID
    assert b'vc_ppg_metrics_f32' in lib.vc_last_error()
    assert lib.vc_ppg_metrics_f32(p, p, p, p, 1, 4, 4, 61, p, None, 4, None, p, p, None) == INVALID          # path without its length
    assert lib.vc_ppg_metrics_f32(p, p, p, p, 1, 4, 4, 0, None, None, 0, None, p, p, None) == INVALID
    assert lib.vc_ppg_metrics_f32(p, p, p, p, 1, 4, 4, 257, None, None, 0, None, p, p, None) == UNSUPPORTED
    assert lib.vc_ppg_metrics_f32(p, p, p, p, 65536, 4, 4, 61, None, None, 0, None, p, p, None) == UNSUPPORTED
    assert lib.vc_ppg_metrics_f32(p, p, p, p, 1, 2 ** 30 + 1, 4, 61, None, None, 0, None, p, p, None) == UNSUPPORTED
    assert lib.vc_phn_segments(p, None, 1, 4, 61, 3, None, p, p, p, p, None) == INVALID and b'vc_phn_segments' in lib.vc_last_error()
    assert lib.vc_phn_segments(p, p, 1, 4, 61, 0, None, p, p, p, p, None) == INVALID                          # min_run < 1
    assert lib.vc_phn_segments(p, p, 1, 4, 257, 3, None, p, p, p, p, None) == UNSUPPORTED
    assert lib.vc_phn_segments(p, p, 1, 2 ** 30 + 1, 61, 3, None, p, p, p, p, None) == UNSUPPORTED
    assert lib.vc_edit_distance_i32(p, p, p, p, 1, 8, 8, p, p, None, 0, None) == INVALID and b'vc_edit_distance_i32' in lib.vc_last_error()
    assert lib.vc_edit_distance_i32(p, p, p, p, 1, 16385, 8, p, p, p, 1 << 30, None) == UNSUPPORTED
    assert lib.vc_edit_distance_i32(p, p, p, p, 1, 8, 8, p, p, p, 16, None) == WORKSPACE


def test_every_host_side_value_error():
    import torch
    import evaluation as ev
    ok = np.zeros((2, 5, 61), np.float32)
    seq = np.zeros((2, 5), np.int32)
    cases = [
        lambda: ev.ppg_metrics_batch(ok[0], ok, [5, 5], [5, 5]),                                    # not [B, F, C]
        lambda: ev.ppg_metrics_batch(ok.astype(np.float64), ok, [5, 5], [5, 5]),                    # dtype
        lambda: ev.ppg_metrics_batch(ok, ok[:1], [5, 5], [5]),                                      # B differs
        lambda: ev.ppg_metrics_batch(ok, ok[:, :, :60], [5, 5], [5, 5]),                            # C differs
        lambda: ev.ppg_metrics_batch(np.zeros((1, 2, 257), np.float32), np.zeros((1, 2, 257), np.float32), [2], [2]),
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 6], [5, 5]),                                       # a length beyond F
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 0], [5, 5]),                                       # a length below 1
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 5], [5, 5], path=torch.zeros((2, 4, 2), dtype=torch.int32)),       # no path_len
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 5], [5, 5], path=torch.zeros((2, 4, 2), dtype=torch.int64),
                                     path_len=torch.zeros(2, dtype=torch.int32)),
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 5], [5, 5], path=torch.zeros((2, 4, 3), dtype=torch.int32),
                                     path_len=torch.zeros(2, dtype=torch.int32)),
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 5], [5, 5], class_map=np.zeros(60, np.int32)),     # map shape
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 5], [5, 5], class_map=np.full(61, 61, np.int32)),  # map range
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 5], [5, 5], class_map=np.full(61, -2, np.int32)),
        lambda: ev.ppg_metrics_batch(ok, ok, [5, 5], [5, 5], class_map=np.zeros(61, np.float32)),   # map dtype
        lambda: ev.phn_segments_batch(ok[0], [5, 5]),
        lambda: ev.phn_segments_batch(ok, [5, 6]),
        lambda: ev.phn_segments_batch(ok, [5, -1]),
        lambda: ev.phn_segments_batch(ok, [5]),
        lambda: ev.phn_segments_batch(ok, [5, 5], min_run=0),
        lambda: ev.phn_segments_batch(ok, [5, 5], min_run=2.0),
        lambda: ev.phn_segments_batch(ok, [5, 5], min_run=True),
        lambda: ev.phn_segments_batch(ok, [5, 5], class_map=np.full(61, 61, np.int32)),
        lambda: ev.edit_distance_batch(seq[0], seq, [5, 5], [5, 5]),
        lambda: ev.edit_distance_batch(seq.astype(np.int64), seq, [5, 5], [5, 5]),
        lambda: ev.edit_distance_batch(seq, seq[:1], [5, 5], [5]),
        lambda: ev.edit_distance_batch(seq, seq, [5, 6], [5, 5]),
        lambda: ev.edit_distance_batch(seq, seq, [5, 5], [-1, 5]),
        lambda: ev.edit_distance_batch(np.zeros((1, 16385), np.int32), seq[:1], [5], [5]),
        lambda: ev.content_batch(ok, ok[:, :, :60], [5, 5], [5, 5]),
        lambda: ev.content_batch(ok, ok, [5, 5], [5, 7]),
        lambda: ev.content_batch(ok, ok, [5, 5], [5, 5], min_run=0),
        lambda: ev.content_batch(ok, ok, [5, 5], [5, 5], class_map=np.zeros(3, np.int32)),
        lambda: ev.content_batch(ok, ok, [5, 5], [5, 5], mask_a=np.ones((2, 4), np.uint8)),         # mask shape
        lambda: ev.content_batch(ok, ok, [5, 5], [5, 5], mask_b=np.ones((2, 5), np.float32)),       # mask dtype
        lambda: ev.content_batch(ok, ok, [5, 5], [5, 5], path_len=torch.zeros(2, dtype=torch.int32)),
        lambda: ev.content_batch(np.zeros((1, 16385, 2), np.float32), np.zeros((1, 4, 2), np.float32), [4], [4]),
        lambda: ev.content_wav_batch(None, np.zeros((1, 8000), np.float32), [8000], np.zeros((1, 8000), np.float32), [8000], None),
    ]
    for c in cases:
        with pytest.raises(ValueError):
            c()


def test_content_wav_batch_checks_its_arguments_on_the_host():
    import evaluation as ev
    from test_mcd_cpu import CFG

    class Enc:
        cfg_d = {'n_output': 61}
    cfg = dict(CFG, n_timesteps=400)
    w = np.zeros((2, 16000), np.float32)
    bad = [
        lambda: ev.content_wav_batch(Enc, w, [16000, 16000], w[:1], [16000], cfg),                          # B differs
        lambda: ev.content_wav_batch(Enc, w, [16000, 16001], w, [16000, 16000], cfg),                       # a length beyond Lmax
        lambda: ev.content_wav_batch(Enc, w, [16000, 100], w, [16000, 16000], cfg),                         # shorter than n_fft // 2
        lambda: ev.content_wav_batch(Enc, w, None, w, None, cfg, align='path'),
        lambda: ev.content_wav_batch(Enc, w, None, w, None, cfg, min_run=0),
        lambda: ev.content_wav_batch(Enc, w, None, w, None, cfg, window_batch=0),
        lambda: ev.content_wav_batch(Enc, w, None, w, None, cfg, mask='loud'),
        lambda: ev.content_wav_batch(Enc, w, None, w, None, cfg, class_map=np.zeros(43, np.int32)),
        lambda: ev.content_wav_batch(Enc, w, None, w, None, cfg, ppg_a=np.zeros((2, 400, 43), np.float32)),
        lambda: ev.content_wav_batch(Enc, w, None, w, None, cfg, res_type='nearest'),
    ]
    for c in bad:
        with pytest.raises(ValueError):
            c()
