"""Speech-activity masks without a GPU: the host reference tests/activity_ref.py against hand-written cases, the host checks
of the new arguments of evaluation.py (made before any launch), and the new exports in the header and the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import activity_ref as ar
from conftest import ROOT
from test_mcd_cpu import CFG


def _m(s):
    return np.array([c == '1' for c in s])


def _s(m):
    return ''.join('1' if v else '0' for v in m)


def test_gaps_of_max_gap_are_filled_and_longer_ones_are_not():
    assert _s(ar.smooth(_m('0110001100001'), max_gap=3, min_run=0)) == '0111111100001'
    assert _s(ar.smooth(_m('0110001100001'), max_gap=4, min_run=0)) == '0111111111111'
    assert _s(ar.smooth(_m('0110001100001'), max_gap=2, min_run=0)) == '0110001100001'
    # a gap at either end has an active frame on one side only: never filled
    assert _s(ar.smooth(_m('0010100'), max_gap=5, min_run=0)) == '0011100'
    assert _s(ar.smooth(_m('0110001100001'), max_gap=0, min_run=0)) == '0110001100001'      # the identity


def test_runs_shorter_than_min_run_are_dropped_after_the_fill():
    assert _s(ar.smooth(_m('0111001100'), max_gap=0, min_run=3)) == '0111000000'              # 3 stays, 2 goes
    assert _s(ar.smooth(_m('0111001100'), max_gap=0, min_run=4)) == '0000000000'
    assert _s(ar.smooth(_m('1100011101'), max_gap=0, min_run=2)) == '1100011100'              # runs touching either end: own length
    assert _s(ar.smooth(_m('1100011101'), max_gap=0, min_run=3)) == '0000011100'
    # the fill comes first: 11 0 1 becomes a run of four, which min_run = 4 keeps
    assert _s(ar.smooth(_m('0110100'), max_gap=1, min_run=4)) == '0111100'
    assert _s(ar.smooth(_m('0110100'), max_gap=0, min_run=4)) == '0000000'
    assert _s(ar.smooth(_m('0110100'), max_gap=0, min_run=1)) == '0110100'


def test_compaction_intervals_and_the_fallback():
    c = ar.compact(_m('0110001101'))
    assert c['index'].tolist() == [1, 2, 6, 7, 9] and c['n_active'] == c['n_kept'] == 5
    assert c['intervals'].tolist() == [[1, 3], [6, 8], [9, 10]]
    c = ar.compact(_m('1111'))                                            # all active: one interval over everything
    assert c['index'].tolist() == [0, 1, 2, 3] and c['n_active'] == 4 and c['intervals'].tolist() == [[0, 4]]
    c = ar.compact(_m('00000'))                                           # none active: everything kept, no interval invented
    assert c['index'].tolist() == [0, 1, 2, 3, 4] and c['n_active'] == 0 and c['n_kept'] == 5 and len(c['intervals']) == 0
    c = ar.compact(_m('1010101'))                                         # the most intervals a row can hold: (F + 1) // 2
    assert len(c['intervals']) == 4
    # the AND over rows of unequal length: frames beyond the shorter row are inactive
    c = ar.compact(_m('0111011111'), _m('110110'))
    assert c['index'].tolist() == [1, 3] and c['n_active'] == 2 and c['intervals'].tolist() == [[1, 2], [3, 4]]
    c = ar.compact(_m('0001111'), _m('111'))                              # nothing in common: the common frames are kept
    assert c['n_active'] == 0 and c['index'].tolist() == [0, 1, 2]


def test_energy_definition_raw_decision_and_path_map():
    x = np.zeros(800, np.float32)
    x[400:] = 0.5
    e = ar.frame_energy(x, hop=80, W=400)
    assert len(e) == 11 and e[0] == 0.0 and e[10] == 0.25 * 200            # frame 10 reads [600, 1000): 200 samples exist
    assert e[5] == 0.25 * 200 and e[8] == 0.25 * 360                       # frame 5 straddles the step; frame 8 reads [440, 840)
    e32 = ar.frame_energy(x, hop=80, W=400, dtype=np.float32)
    assert e32.dtype == np.float32 and np.array_equal(e32.astype(np.float64), e)      # small dyadic sums are exact in float32
    rng = np.random.RandomState(0)
    y = rng.standard_normal(3000).astype(np.float32)
    e64, e32 = ar.frame_energy(y), ar.frame_energy(y, dtype=np.float32)
    assert np.abs(e32 / e64 - 1).max() < 400 * 2.0 ** -24
    raw, marg = ar.raw_energy(np.array([0.0, 1.0, 1.00001e-4, 1.1e-4, 0.9e-4, 0.5]), top_db=40.0)
    assert raw.tolist() == [False, True, True, True, False, True] and marg.tolist() == [False, False, True, False, False, False]
    assert not ar.raw_energy(np.zeros(4))[0].any()                          # digital silence: e > 0 fails
    assert ar.ratio(40.0) == np.float32(1e-4)
    p = ar.path_map([[0, 0], [1, 0], [2, 1]], [3, 5, 8], [2, 9])
    assert p.tolist() == [[3, 2], [5, 2], [8, 9]]


def test_speech_gain_is_taken_over_the_samples_of_active_frames():
    x = np.concatenate([np.full(400, 0.5), np.full(400, -0.001)]).astype(np.float32)          # 11 frames of hop 80
    m = _m('11111000000')                                                   # frames 0 .. 4 own the samples [0, 360)
    assert ar.speech_gain(x, m, 80, 0.003) == pytest.approx(0.003 / 0.5, rel=1e-12)
    m = _m('00000000011')                                                   # frame 9 from sample 680 on, frame 10 the rest
    assert ar.speech_gain(x, m, 80, 0.003) == pytest.approx(0.003 / float(np.float32(0.001)), rel=1e-12)
    whole = 0.003 / np.abs(x.astype(np.float64)).mean()
    assert ar.speech_gain(x, _m('00000000000'), 80, 0.003) == pytest.approx(whole, rel=1e-12)      # no active frame: all samples
    assert ar.speech_gain(x, _m('11111111111'), 80, 0.003) == pytest.approx(whole, rel=1e-12)
    assert ar.speech_gain(np.zeros(800, np.float32), _m('11111111111')) == 1.0
    # the same speech with silence around it gets the same gain, which the whole-waveform normalisation does not give
    a, b, _ = ar.silence_pair(31)
    ga, gb = ar.speech_gain(a, ar.activity(a)['mask']), ar.speech_gain(b, ar.activity(b)['mask'])
    assert abs(gb / ga - 1) < 0.03 and (0.003 / np.abs(b).mean()) / (0.003 / np.abs(a).mean()) > 2.0


def test_a_tone_with_a_pause_gives_two_intervals_or_one():
    x = np.zeros(16000, np.float32)
    t = np.arange(16000) / 16000.0
    x[:6000] = 0.3 * np.sin(2 * np.pi * 200 * t[:6000])
    x[10000:] = 0.3 * np.sin(2 * np.pi * 200 * t[10000:])
    a = ar.activity(x, max_gap=20)
    assert len(a['intervals']) == 2 and a['intervals'][0][0] == 0 and a['intervals'][1][1] == 201
    assert abs(a['intervals'][0][1] - 6000 / 80) <= 3 and abs(a['intervals'][1][0] - 10000 / 80) <= 3
    assert len(ar.activity(x, max_gap=60)['intervals']) == 1               # a 46-frame pause is a gap to max_gap = 60


def test_host_checks_of_the_new_arguments():
    """Every check is made before anything is launched: these raise ValueError on a machine without a GPU."""
    import evaluation as ev
    wav = np.zeros((2, 1600), np.float32)
    with pytest.raises(ValueError, match='mode'):
        ev.activity_batch(wav, mode='loud')
    with pytest.raises(ValueError, match='max_gap'):
        ev.activity_batch(wav, max_gap=-1)
    with pytest.raises(ValueError, match='min_run'):
        ev.activity_batch(wav, min_run=1.5)
    for bad in (0.0, -3.0, float('inf'), float('nan'), 1000.0):              # 10^-100 is no float32
        with pytest.raises(ValueError, match='top_db'):
            ev.activity_batch(wav, top_db=bad)
    with pytest.raises(ValueError, match='frame_length'):
        ev.activity_batch(wav, frame_length=0)
    with pytest.raises(ValueError, match='16384'):
        ev.activity_batch(np.zeros((1, 16384 * 80), np.float32))            # 16385 frames
    with pytest.raises(ValueError, match='f0'):
        ev.activity_batch(wav, mode='voiced', f0=np.zeros((2, 5), np.float32))
    mel = np.zeros((2, 30, 80), np.float32)
    ok = np.ones((2, 30), np.uint8)
    with pytest.raises(ValueError, match='mask_a'):
        ev.mcd_batch(mel, mel, [30, 30], [30, 30], CFG, mask_a=np.ones((2, 29), np.uint8), mask_b=ok)
    with pytest.raises(ValueError, match='mask_b'):
        ev.mcd_batch(mel, mel, [30, 30], [30, 30], CFG, mask_a=ok, mask_b=np.ones((2, 30), np.float32))
    with pytest.raises(ValueError, match='mask_b'):
        ev.mcd_batch(mel, mel, [30, 30], [30, 30], CFG, mask_b=np.ones((30,), np.uint8))
    w = np.zeros((1, 4000), np.float32)
    for call in (ev.mcd_wav_batch, ev.score_wav_batch):
        with pytest.raises(ValueError, match='mode'):
            call(w, None, w, None, CFG, mask='speech')
        with pytest.raises(ValueError, match='max_gap'):
            call(w, None, w, None, CFG, mask='energy', max_gap=-2)
        with pytest.raises(ValueError, match='top_db'):
            call(w, None, w, None, CFG, mask='energy', top_db=0)
    with pytest.raises(ValueError, match='index'):
        ev.compact_batch(np.zeros((1, 4, 3), np.float32), np.zeros((1, 4), np.int32), np.zeros((1,), np.int32))
    assert ev._activity_args('energy+voiced', 40.0, 20, 0, 't') == (3, float(np.float32(1e-4)), 20, 0)
    assert ev._SCORE._fields[-4:] == ('n_active_a', 'n_active_b', 'mask_a', 'mask_b') and ev._SCORE._fields[:4] == ('mcd', 'total', 'path_len', 'path')


NEW = ('vc_frame_energy_tile', 'vc_frame_energy_f32', 'vc_activity_mask', 'vc_mask_compact', 'vc_compact_rows_f32', 'vc_path_map',
       'vc_speech_gain_f32', 'vc_scale_rows_f32')


def test_the_new_exports_are_declared_bound_and_validate_on_the_host():
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _vc.lib()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _vc._SIGS and hasattr(lib, name), name
    assert os.path.exists(os.path.join(ROOT, 'speech-cloner_amd', 'csrc', 'vc_activity.hip'))
    # the tile of the energy kernel: 64 frames while frame_length + 63 hop samples fit 64 KB, halved beyond; host arithmetic
    assert lib.vc_frame_energy_tile(80, 400) == 64 and lib.vc_frame_energy_tile(512, 400) == 32 and lib.vc_frame_energy_tile(65536, 8192) == 1
    assert lib.vc_frame_energy_tile(0, 400) == 0 and lib.vc_frame_energy_tile(80, 8193) == 0
    # arguments are refused before any HIP call
    assert lib.vc_frame_energy_f32(None, None, 1, 100, 100, 80, 400, None, 2, None) == 1 and b'vc_frame_energy_f32' in lib.vc_last_error()
    p = ctypes.c_void_p(4096)                                             # (never dereferenced)
    assert lib.vc_activity_mask(p, None, p, 1, 16385, 1, 1e-4, 20, 0, p, None) == 4 and b'16384' in lib.vc_last_error()
    assert lib.vc_activity_mask(p, None, p, 1, 100, 3, 1e-4, 20, 0, p, None) == 1 and b'd_f0' in lib.vc_last_error()
    assert lib.vc_activity_mask(p, None, p, 1, 100, 1, 0.0, 20, 0, p, None) == 1 and b'ratio' in lib.vc_last_error()
    assert lib.vc_mask_compact(p, p, 100, p, None, 0, 1, p, p, p, p, p, None) == 1 and b'vc_mask_compact' in lib.vc_last_error()
    assert lib.vc_compact_rows_f32(p, 100, p, 100, p, 1, 5000, p, 100, None) == 4
    assert lib.vc_path_map(None, None, 1, 10, p, 5, p, 5, p, None) == 1
