"""The general front-end's float64 reference (tests/frontend_general_ref.py) and the inputs of its device tests, checked
without a device: against oracle/frontend_oracle.py, against the library's host tables, against the launcher's formulas
as this file restates them, for float32 headroom, and for exactness of the hand-written stage-3 data."""
import functools

import numpy as np
import pytest

from oracle import frontend_oracle as fo
import frontend_general_cases as fc
import frontend_general_ref as ref


@functools.lru_cache(maxsize=None)
def _stage2(cid, pre):
    kw = dict(fc.kw_of(cid), pre_emphasis=pre)
    wav, lens = fc.inputs(cid)
    return tuple(ref.stage2(wav[b, :L], kw) for b, L in enumerate(lens))


def test_cases_are_the_listed_ones():
    assert len(fc.IDS) == 14 and fc.CASES['big-finalize-128'][0]['n_mfcc'] == 128
    for cid in fc.IDS:
        kw = fc.kw_of(cid)
        wav, lens = fc.inputs(cid)
        n_fft, hop = ref.n_fft_of(kw), kw['hop_length']
        G = ref.tile_frames(n_fft)
        F = [ref.num_frames(L, hop) for L in lens]
        assert len(lens) >= 4 and min(lens) > n_fft // 2 and min(F) >= 2
        assert len(set(L % hop for L in lens)) > 1                       # the remainder is not always 0
        want = fc.frame_counts(kw)
        assert all(f == w or (f > w and lens[b] <= n_fft // 2 + 1 + b) for b, (f, w) in enumerate(zip(F, want)))
        assert {G, G + 1, 2 * G + 1} <= set(F)
        assert max(F) - min(F) >= G                                      # the shortest is padded by whole tiles
        assert n_fft != 2048 or max(F) <= 20
        for b, L in enumerate(lens):
            assert np.abs(wav[b, :L]).max() > 0 and not wav[b, L:].any()
        run = n_fft + 2 * hop
        x = wav[4, :lens[4]]
        zero_runs = np.diff(np.flatnonzero(np.concatenate([[1], x != 0, [1]])))
        assert zero_runs.max() - 1 >= run                                # digital silence inside
        assert wav[3, lens[3] - 1] == 1.0                                # the click sits in the last frame
    for cid in fc.IDS:
        names = [n for n, _ in fc.variants(cid)]
        assert names == (list(fc.FLAG_SETS) if cid in fc.ALL_FLAG_IDS else ['listed', 'opposite'])
    for k in fc.FLAG_SETS['A']:
        assert len({repr(f[k]) for f in fc.FLAG_SETS.values()}) == 2, k
    assert fc.opposite(fc.FLAG_SETS['A']) == fc.FLAG_SETS['B']


@pytest.mark.parametrize('cid,name', fc.ALL_VARIANTS, ids=['%s-%s' % v for v in fc.ALL_VARIANTS])
def test_reference_agrees_with_oracle(cid, name):
    """Stages 2 and 3 composed equal calc_MFCC_input of the oracle, which rounds the spectrum to complex64: 1e-6 on outputs
    scaled by 0.01, 1e-4 on unit factors.  The oracle is handed the float32 samples widened to float64, so that it keeps the
    SCALED signal (y * norm / mean|y|) in float64 as well.  Handed float32 it rounds that product to float32, white noise
    144 dB under the signal that reaches the bins near the top_db floor: measured on these inputs with
    mean_abs_amp_norm = 0.003, the scaled power then differs by up to 2.3e-5 (one-cep), 6.8e-6 (ref-defaults), 3.5e-6
    (hop160), where it is 1.5e-7 on the widened samples; MFCC, mel and every unit-factor output are the same either way."""
    kw = fc.variant_kw(cid, name)
    wav, lens = fc.inputs(cid)
    s2 = _stage2(cid, kw['pre_emphasis'])
    worst = 0.0
    for b, L in enumerate(lens):
        x = wav[b, :L]
        got = ref.stage3(s2[b][0], s2[b][1], s2[b][2], ref.abssum_partials(x), L, kw)
        want = fo.calc_MFCC_input(x.astype(np.float64), **kw)
        for n, g, w in zip(('mfcc', 'mel', 'pow'), got, want):
            bound = 1e-4 if fc.tol(n, kw) == fc.DB_TOL[n] else 1e-6
            assert g.shape == w.shape, (n, g.shape, w.shape)
            err = np.abs(g - w).max()
            worst = max(worst, err / bound)
            assert err <= bound, (cid, name, b, n, err, bound)
    print('MEASURED %s-%s reference vs oracle: worst error / bound %.3f' % (cid, name, worst))


def test_stage1_and_tile_sums_add_up():
    for cid in fc.IDS:
        kw = fc.kw_of(cid)
        wav, lens = fc.inputs(cid)
        for b, L in enumerate(lens):
            total = np.abs(wav[b, :L].astype(np.float64)).sum()
            assert abs(ref.abssum_partials(wav[b, :L]).sum() - total) <= 1e-12 * total
            if ref.fused_abs(kw):
                assert abs(_stage2(cid, kw['pre_emphasis'])[b][2][:, 4].sum() - total) <= 1e-12 * total


@pytest.mark.parametrize('cid', fc.IDS)
def test_host_tables_equal_the_reference(cid):
    import audio_lib
    kw = fc.kw_of(cid)
    n_fft = ref.n_fft_of(kw)
    mel, dct = audio_lib.host_tables(kw['sr'], n_fft, kw['n_mels'], kw['n_mfcc'])
    rmel, rdct = ref.mel_matrix(kw['sr'], n_fft, kw['n_mels']), ref.dct_matrix(kw['n_mfcc'], kw['n_mels'])
    assert np.array_equal(mel != 0, rmel != 0)
    assert np.abs(mel - rmel).max() <= 1e-12 * np.abs(rmel).max() and np.abs(dct - rdct).max() <= 1e-14
    assert np.abs(mel - fo.mel_filterbank(kw['sr'], n_fft, kw['n_mels'])).max() <= 1e-12 * np.abs(rmel).max()
    assert np.abs(dct - fo.dct_basis(kw['n_mfcc'], kw['n_mels'])).max() <= 1e-14
    assert ref.sparse_mel(mel)[2:] == fc.TABLE_FACTS[cid]


def test_table_facts_are_the_listed_ones():
    f = fc.TABLE_FACTS
    assert f['hop160'][:2] == (391, 14) and f['sr22050'][1] == 16 and f['sr8000'][1] == 12
    assert f['wide-mel'][2] == 47 and f['tiny-empty'][2] == 7
    assert [cid for cid in fc.IDS if f[cid][2]] == ['wide-mel', 'tiny-empty']


def test_launcher_formulas_restated():
    over = {}
    for cid in fc.IDS:
        kw, route, big, _ = fc.CASES[cid]
        assert ref.routing(kw) == route, cid
        lds = ref.lds_bytes(kw)
        assert 0 < lds['power'] <= ref.LDS_MAX and 0 < lds['finalize'] <= ref.LDS_MAX, (cid, lds)
        if route != 'fast400':
            assert tuple(k for k in ('power', 'finalize') if lds[k] > ref.LDS_OPT_IN) == big, (cid, lds)
            over.update({cid: {k: lds[k] for k in big}} if big else {})
            assert lds['alias'] == (route == 'power400' and cid != 'wide-mel'), cid
        assert ref.fused_abs(kw) == (cid not in fc.ABSSUM_IDS), cid
    assert over == fc.LDS_FACTS
    assert fc.OVER_64K == ('big-finalize-80', 'big-finalize-128', 'big-power400', 'max-fft')
    # the workspace: partials | records | mel, 256-byte aligned, no counter block
    kw = fc.kw_of('tiny')
    assert ref.ws_layout(kw, 3, 100) == (0, 256, 256 + 256, 512 + 1024, 1, 7)
    assert ref.ws_layout(fc.kw_of('hop160'), 7, 10398)[1:] == (512, 512 + 1280, 1792 + align(7 * 65 * 80 * 4), 5, 65)


def align(v):
    return (v + 255) & ~255


@pytest.mark.parametrize('cid', fc.IDS)
def test_float32_headroom_of_the_inputs(cid):
    """A float32 stage 2 at its most pessimistic (one sequential sum per bin, float32 twiddles) stays within 1/4 of the
    device's tolerance above the top_db floor on every input, with and without pre-emphasis."""
    wav, lens = fc.inputs(cid)
    worst = {'pow': 0.0, 'mel': 0.0}
    for pre in (0.0, 0.97):
        kw = dict(fc.kw_of(cid), pre_emphasis=pre)
        for b, L in enumerate(lens):
            p64, m64, _ = _stage2(cid, pre)[b]
            p32, m32 = ref.stage2_f32_sequential(wav[b, :L], kw)
            for n, a, r_, fl in zip(('pow', 'mel'), (p32, m32), (p64, m64), ref.floors(p64, m64)):
                err = np.abs(np.maximum(a, fl) - np.maximum(r_, fl)).max()
                worst[n] = max(worst[n], err)
                assert err <= fc.DB_TOL[n] / 4, (cid, pre, b, n, err)
    print('MEASURED %s float32 model: pow %.2e / %.1e dB, mel %.2e / %.1e dB'
          % (cid, worst['pow'], fc.DB_TOL['pow'] / 4, worst['mel'], fc.DB_TOL['mel'] / 4))


def _is_f32(v):
    v = np.asarray(v, dtype=np.float64)
    return np.array_equal(v.astype(np.float32).astype(np.float64), v)


@pytest.mark.parametrize('cid', fc.EXACT_IDS)
@pytest.mark.parametrize('name', fc.EXACT_SETS)
def test_exact_stage3_cases_are_exactly_representable(cid, name):
    """On the hand-written data every intermediate of the power and mel outputs is a float32 number: the raw values, the
    floors and minima (multiples of 1/8 below 2^10), the differences, and their products with 1/128."""
    kw = fc.exact_kw(cid)
    G = ref.tile_frames(ref.n_fft_of(kw))
    data = fc.exact_data(cid, name)
    outs = []
    for b, L in enumerate(fc.exact_lens(cid)):
        p, m = data[b]
        F = ref.num_frames(L, kw['hop_length'])
        assert p.shape[0] == F and m.shape == (F, kw['n_mels'])
        rec = ref.tile_records(p, m, np.zeros((F + G - 1) // G), G, (F + G - 1) // G)
        for a, (imax, imin) in ((p, (0, 1)), (m, (2, 3))):
            assert np.array_equal(a * 8, np.round(a * 8)) and np.abs(a).max() < 1024
            hi, lo = max(rec[:, imax].max(), -100.0), max(rec[:, imin].min(), -100.0)
            floor = max(hi - 80.0, -100.0)
            lo_c = max(lo, floor)
            w = np.maximum(a, floor)
            assert _is_f32(w) and _is_f32(w - lo_c) and _is_f32(fc.EXACT_FACTOR * (w - lo_c))
            if name == 'range120':
                assert lo_c == floor and floor > a.min()
            elif name in ('range30', 'nan_padding'):
                assert lo_c == a.min() > floor
            elif name == 'below_amin':
                assert floor == -100.0 and lo_c == -100.0 and a.max() < -100.0
        c, mo, po = ref.stage3(p, m, rec, None, L, kw)
        assert _is_f32(mo) and _is_f32(po) and mo.min() == 0.0 and po.min() == 0.0
        if name == 'below_amin':
            # (the cepstra of a constant row: the cosine rows sum to 0 up to rounding, the first one goes with frame 0's)
            assert np.abs(c).max() < 1e-12 and not mo.any() and not po.any()
        outs.append((c, mo, po))
    if name == 'late_max':
        assert np.array_equal(data[2][0][:G + 1], data[1][0]) and np.array_equal(data[2][1][:G + 1], data[1][1])
        assert not outs[2][1][:G + 1].any() and not outs[2][2][:G + 1].any()     # under the floor of utterance 2 ...
        assert outs[1][1].max() > 0.2 and outs[1][2].max() > 0.2                 # ... and well above the minimum of 1
