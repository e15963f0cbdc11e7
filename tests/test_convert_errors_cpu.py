"""The errors of conversion.py's seven batched entry points, pinned (no GPU): every call of CALLS raises exactly the
exception type and message recorded in tests/golden/convert_errors.json.  The fixture was recorded once from the
conversion.py that still held one copy of every check per entry point (the commit before the checks were folded into
shared helpers), never from the code under test, so it pins the message texts and, where a call has two bad arguments,
which of them is reported first.  A fully valid call ends in VCError('... needs a GPU') on a machine without one: nothing
before that line may touch the decoder or the device."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_convert_batch_cpu import CFG

FIXTURE = os.path.join(GOLDEN, 'convert_errors.json')


class _NoDecoder:
    encoder = object()

    def __getattr__(self, name):
        raise AssertionError('the decoder was touched before validation finished')


class _Encoder:
    cfg_d = {'n_output': 61}


class _DecodeDecoder(_NoDecoder):
    """segments='decode' reads the class count from the encoder's configuration, and nothing else."""
    encoder = _Encoder()


WAV = np.zeros((3, 80000), np.float32)                            # 1001, 501, 751 frames -> 1200, 800, 800 stitched: Fout = 1200
LENS = [80000, 40000, 60000]
LONG = np.zeros((1, 80 * 16400), np.float32)                      # 16,800 stitched frames: past the warp's 16,384
BAD_LENS = [80000, 90000, 100]
STATS = (10, 5.0, 0.2)
TABLE = tuple(np.zeros(s, np.int32) for s in ((3, 4), (3, 4), (3, 4), (3,)))


def _calls():
    """(name, entry point, decoder stand-in, wav, keyword arguments).  The names are the fixture's keys."""
    out = []

    def add(entry, name, wav=WAV, dec=_NoDecoder, lens=LENS, cfg_d=CFG, **kw):
        out.append(('{}:{}'.format(entry, name), 'convert_' + entry, dec, wav, dict(kw, lens=lens, cfg_d=cfg_d)))

    phase_bad = np.zeros((3, 400, 201), np.float32)
    contour_bad = np.zeros((3, 400), np.float32)

    # ---- the preamble, the phase argument and a plan error, for the entries that take them
    for entry, kw in (('batch', {}), ('duration_batch', dict(rate=1.25)), ('pitch_batch', dict(pitch=1.2)),
                      ('postfilter_batch', dict(model=object()))):
        add(entry, 'valid', **kw)
        add(entry, 'no cfg_d', cfg_d=None, **kw)
        add(entry, 'no cfg_d, bad momentum', cfg_d=None, momentum=1.5, **kw)
        add(entry, 'no cfg_d, bad phase', cfg_d=None, phase='host', **kw)
        add(entry, 'phase string', phase='host', **kw)
        add(entry, 'phase numpy', phase='numpy', **kw)
        add(entry, 'phase string, bad lens', phase='host', lens=BAD_LENS, **kw)
        add(entry, 'phase shape', phase=phase_bad, **kw)
        add(entry, 'phase shape, empty span', phase=phase_bad, lens=[80000, 30000, 60000], t_s=2, **kw)
        add(entry, 'phase shape, bad utt_ids', phase=phase_bad, utt_ids=[0, 1], **kw)
        add(entry, 'phase of the right shape', phase=np.zeros((3, 1200, 201), np.float32), **kw)
        add(entry, 'bad lens', lens=BAD_LENS, **kw)
        add(entry, 'wav not 2-d', wav=WAV[0], **kw)
        add(entry, 'both encoders', encoder=object(), **kw)
        add(entry, 'resampled both ways', wav_sr=22050, out_sr=8000, lens=[80000, 60000, 70000], **kw)
    add('batch', 'vocode off', vocode=False)
    add('batch', 'vocode off, phase shape', vocode=False, phase=phase_bad)
    add('postfilter_batch', 'no model', phase='host')
    add('postfilter_batch', 'bad mode, phase string', model=object(), mode='sm', phase='host')
    add('postfilter_batch', 'bad mode, bad lens', model=object(), mode='sm', lens=BAD_LENS)

    # ---- the duration request
    for entry in ('duration_batch', 'diff_duration_batch'):
        dd = entry == 'diff_duration_batch'
        add(entry, 'no cfg_d, no request', cfg_d=None)
        add(entry, 'no request')
        add(entry, 'two requests', rate=1.0, ratio=[1.0])
        add(entry, 'two requests, bad lens', rate=1.0, out_len=TABLE[0], lens=BAD_LENS)
        add(entry, 'rate zero', rate=0.0)
        add(entry, 'rate bool', rate=True)
        add(entry, 'rate too large, bad gap_ratio', rate=8.5, gap_ratio=-1.0)
        add(entry, 'bad gap_ratio', rate=1.0, gap_ratio=9.0)
        add(entry, 'bad gap_ratio, bad segments', ratio=[1.0], gap_ratio='x', segments='align')
        add(entry, 'segments string', ratio=[1.0], segments='align')
        add(entry, 'segments of three', ratio=[1.0], segments=TABLE[:3])
        add(entry, 'segments ignored with rate', rate=1.0, segments='align')
        add(entry, 'decode with rate', rate=1.0, decode=dict(min_dur=2))
        add(entry, 'decode with a table', ratio=[1.0], segments=TABLE, decode={})
        add(entry, 'decode keys', ratio=[1.0], decode=dict(bogus=1, kind='prob'), dec=_DecodeDecoder)
        add(entry, 'decode keys, bad max_frames', ratio=[1.0], decode=dict(bogus=1), max_frames=-1, dec=_DecodeDecoder)
        add(entry, 'decode keys, bad lens', ratio=[1.0], decode=dict(bogus=1), lens=BAD_LENS, dec=_DecodeDecoder)
        add(entry, 'decode value, bad max_frames', ratio=[1.0], decode=dict(min_dur=0), max_frames=1, dec=_DecodeDecoder)
        add(entry, 'decode value', ratio=[1.0], decode=dict(min_dur=0), dec=_DecodeDecoder)
        add(entry, 'decode penalty', ratio=[1.0], decode=dict(penalty=float('nan')), dec=_DecodeDecoder)
        add(entry, 'decode class_map', ratio=[1.0], decode=dict(class_map=[0, 1]), dec=_DecodeDecoder)
        add(entry, 'decode class_map, bad min_dur', ratio=[1.0], decode=dict(class_map=[0, 1], min_dur=0), dec=_DecodeDecoder)
        add(entry, 'bad lens, bad ratio', ratio=[9.0], lens=BAD_LENS, segments=TABLE)
        add(entry, 'too many stitched frames', wav=LONG, lens=[LONG.shape[1]], rate=1.0, t_e=100)
        add(entry, 'too many stitched frames, bad max_frames', wav=LONG, lens=[LONG.shape[1]], rate=1.0, t_e=100, max_frames=0)
        add(entry, 'rate leaves too few frames', rate=0.001)
        add(entry, 'rate leaves too few frames, bad max_frames', rate=0.001, max_frames=0)
        add(entry, 'host ratio out of range', ratio=[0.5, 9.0], segments=TABLE)
        add(entry, 'host ratio not finite', ratio=[float('nan')], segments=TABLE)
        add(entry, 'host ratio 2-d, bad max_frames', ratio=np.ones((2, 2), np.float32), segments=TABLE, max_frames=0)
        add(entry, 'tensor ratio 2-d', ratio=torch.ones((2, 2)), segments=TABLE, max_frames=1500)
        add(entry, 'tensor ratio of integers', ratio=torch.ones((2,), dtype=torch.int32), segments=TABLE, max_frames=1500)
        add(entry, 'tensor ratio without max_frames', ratio=torch.ones((2,)), segments=TABLE)
        add(entry, 'out_len without max_frames', out_len=TABLE[0], segments=TABLE)
        add(entry, 'max_frames zero', rate=1.0, max_frames=0)
        add(entry, 'max_frames one', rate=1.0, max_frames=1)
        add(entry, 'max_frames float', rate=1.0, max_frames=1500.0)
        add(entry, 'max_frames too large', ratio=[1.0], segments=TABLE, max_frames=16385)
        add(entry, 'max_frames bad, decode value', ratio=[1.0], max_frames=True, decode=dict(min_dur=0), dec=_DecodeDecoder)
        add(entry, 'valid rate', rate=1.25)
        add(entry, 'valid host ratio with a table', ratio=[1.0, 1.5], gap_ratio=0.75, segments=TABLE)
        add(entry, 'valid tensor ratio, decode', ratio=torch.ones((61,)), max_frames=1500, decode=dict(min_dur=2), dec=_DecodeDecoder)
        add(entry, 'valid out_len', out_len=TABLE[0], segments=TABLE, max_frames=1500)
        if dd:
            add(entry, 'bad max_frames, bad group', rate=1.0, max_frames=0, group=0)
            add(entry, 'bad group, decode value', ratio=[1.0], group=0, decode=dict(min_dur=0), dec=_DecodeDecoder)
            add(entry, 'bad alpha', rate=1.0, alpha=2.0)                       # convert_diff_batch's own, after the request
            add(entry, 'no request, bad alpha', alpha=2.0)
            add(entry, 'pitch string', rate=1.0, pitch='target')
            add(entry, 'pitch string, bad max_frames', rate=1.0, pitch='target', max_frames=0)
            add(entry, 'f0_args keys, decode keys', ratio=[1.0], f0_args=dict(bogus=1), decode=dict(bogus=1), dec=_DecodeDecoder)
            add(entry, 'f0_args keys', rate=1.0, f0_args=dict(bogus=1))
            add(entry, 'contour shape', rate=1.0, pitch=contour_bad)
        else:
            add(entry, 'bad mode, no request', mode='cubic')
            add(entry, 'bad mode, phase string', rate=1.0, mode='cubic', phase='host')
            add(entry, 'phase shape at max_frames', rate=1.25, phase=np.zeros((3, 1200, 201), np.float32))
            add(entry, 'phase of the warped shape', rate=1.25, phase=np.zeros((3, 1500, 201), np.float32))
            add(entry, 'phase shape, decode value', ratio=[1.0], phase=phase_bad, decode=dict(min_dur=0), dec=_DecodeDecoder)
            add(entry, 'bad max_frames, phase shape', rate=1.0, max_frames=0, phase=phase_bad)

    # ---- pitch=, the tracker's arguments
    for entry in ('pitch_batch', 'hnm_batch', 'diff_batch'):
        add(entry, 'no cfg_d, pitch string', cfg_d=None, pitch='target')
        add(entry, 'pitch none')
        add(entry, 'pitch string', pitch='target')
        add(entry, 'pitch string, stats apart', pitch='target', stats_src=STATS)
        add(entry, 'pitch string, f0_args keys', pitch='target', f0_args=dict(bogus=1))
        add(entry, 'pitch string, bad lens', pitch='target', lens=BAD_LENS)
        add(entry, 'stats apart', pitch='source', stats_src=STATS)
        add(entry, 'stats apart, ratio out of range', pitch=3.0, stats_tgt=STATS)
        add(entry, 'stats with a ratio', pitch=1.2, stats_src=STATS, stats_tgt=STATS)
        add(entry, 'stats with a contour', pitch=np.zeros((3, 1200), np.float32), stats_src=STATS, stats_tgt=STATS)
        add(entry, 'stats without pitch', stats_src=STATS, stats_tgt=STATS)
        add(entry, 'source', pitch='source')
        add(entry, 'source with stats', pitch='source', stats_src=STATS, stats_tgt=STATS)
        add(entry, 'source with stats of two', pitch='source', stats_src=STATS[:2], stats_tgt=STATS)
        add(entry, 'ratio out of range', pitch=3.0)
        add(entry, 'ratio bool', pitch=True)
        add(entry, 'ratio 0-d array', pitch=np.array(1.2))
        add(entry, 'ratio 0-d array out of range', pitch=np.array(3.0))
        add(entry, 'ratio numpy scalar', pitch=np.float32(1.5))
        add(entry, 'ratio out of range, f0_args keys', pitch=3.0, f0_args=dict(bogus=1))
        if entry != 'hnm_batch':
            add(entry, 'ratio out of range, bad w_floor', pitch=3.0, w_floor=0.0)
            add(entry, 'bad w_floor, f0_args keys', pitch=1.2, w_floor=0.0, f0_args=dict(bogus=1))
        add(entry, 'f0_args keys', pitch=1.2, f0_args=dict(bogus=1, fmin=50.0))
        add(entry, 'f0_args keys without pitch', f0_args=dict(bogus=1))
        add(entry, 'f0_args keys, bad lens', pitch=1.2, f0_args=dict(bogus=1), lens=BAD_LENS)
        add(entry, 'f0_args keys, contour shape', pitch=contour_bad, f0_args=dict(bogus=1))
        add(entry, 'f0_args value', pitch=1.2, f0_args=dict(fmin=-1.0))
        add(entry, 'f0_args value without pitch', f0_args=dict(fmin=-1.0))
        add(entry, 'f0_args value, bad lens', pitch=1.2, f0_args=dict(fmin=-1.0), lens=BAD_LENS)
        add(entry, 'f0_args value, contour shape', pitch=contour_bad, f0_args=dict(fmin=-1.0))
        add(entry, 'f0_args n_cand', pitch='source', stats_src=STATS, stats_tgt=STATS, f0_args=dict(n_cand=0))
        add(entry, 'f0_args jump_cost', pitch='source', stats_src=STATS, stats_tgt=STATS, f0_args=dict(jump_cost=-1.0))
        add(entry, 'f0_args threshold, n_cand', pitch=1.2, f0_args=dict(threshold=-1.0, n_cand=0))
        add(entry, 'contour shape', pitch=contour_bad)
        add(entry, 'contour shape, empty span', pitch=contour_bad, lens=[80000, 30, 60000])
        add(entry, 'contour shape, bad lens', pitch=contour_bad, lens=BAD_LENS)
        add(entry, 'contour', pitch=np.zeros((3, 1200), np.float32))
        add(entry, 'contour tensor', pitch=torch.zeros((3, 1200)))
        add(entry, 'valid ratio', pitch=1.2)
        add(entry, 'valid ratio resampled', pitch=1.2, wav_sr=22050, out_sr=8000, lens=[80000, 60000, 70000])
        add(entry, 'bad lens, no pitch', lens=BAD_LENS)
        add(entry, 'no cfg_d, no pitch', cfg_d=None)
    add('pitch_batch', 'contour shape, phase shape', pitch=contour_bad, phase=phase_bad)
    add('pitch_batch', 'pitch none, phase string', phase='host')
    add('pitch_batch', 'no cfg_d, bad seed', cfg_d=None, pitch=1.2, seed=-1)
    add('hnm_batch', 'no cfg_d, bad seed', cfg_d=None, seed=-1)
    add('hnm_batch', 'contour shape, bad order', pitch=contour_bad, order=0)
    add('hnm_batch', 'contour, f0_args ignored', pitch=np.zeros((3, 1200), np.float32), f0_args=dict(bogus=1))
    add('diff_batch', 'no cfg_d, bad alpha', cfg_d=None, alpha=2.0)
    add('diff_batch', 'bad alpha, pitch string', alpha=2.0, pitch='target')
    add('diff_batch', 'bad half_width, pitch string', half_width=99, pitch='target')
    add('diff_batch', 'too short for the filter', lens=[80000, 40000, 230])
    add('diff_batch', 'too short for the filter, f0_args value', lens=[80000, 40000, 230], pitch=1.2, f0_args=dict(fmin=-1.0))
    return out


CALLS = _calls()


def outcome(fn, dec, wav, kw):
    """(exception type name, message) of one call; (None, None) if it returns."""
    try:
        fn(dec(), wav, **kw)
    except Exception as e:                                         # noqa: BLE001  (the type is what is recorded)
        return type(e).__name__, str(e)
    return None, None


def test_the_list_covers_every_entry_point_and_name_once():
    names = [c[0] for c in CALLS]
    assert len(set(names)) == len(names)
    assert {c[1] for c in CALLS} == {'convert_batch', 'convert_duration_batch', 'convert_pitch_batch', 'convert_hnm_batch',
                                     'convert_diff_batch', 'convert_diff_duration_batch', 'convert_postfilter_batch'}
    recorded = json.load(open(FIXTURE))
    assert [r[0] for r in recorded] == names
    # every entry point has a fully valid call on record, and every other call on record raised something else
    for entry in {c[1] for c in CALLS}:
        assert any(r[1] == 'VCError' and r[2].startswith(entry if entry != 'convert_diff_duration_batch' else 'convert_diff_batch')
                   and 'needs a GPU' in r[2] for r, c in zip(recorded, CALLS) if c[1] == entry), entry
    assert all(r[1] is not None for r in recorded)


@pytest.mark.parametrize('i', range(len(CALLS)), ids=[c[0] for c in CALLS])
def test_error_is_the_recorded_one(i):
    import conversion
    name, entry, dec, wav, kw = CALLS[i]
    rec_name, rec_type, rec_msg = json.load(open(FIXTURE))[i]
    assert rec_name == name
    if rec_type == 'VCError' and 'needs a GPU' in rec_msg and torch.cuda.is_available():
        pytest.skip('a valid call: it runs where a GPU is present')
    assert outcome(getattr(conversion, entry), dec, wav, kw) == (rec_type, rec_msg)
