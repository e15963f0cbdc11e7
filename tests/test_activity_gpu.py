"""The speech-activity launches on the device against tests/activity_ref.py: frame energy of a ragged batch against the
float64 definition, the raw decisions off the threshold, the integer work (smoothing, compaction, intervals, gather,
path map) exactly, the bit-identities (alone / batched, twice, reversed, gain, graph replay), no host synchronisation,
the defaults, masked score_wav_batch against the float64 pipeline, and the property the masks exist for."""
import numpy as np
import pytest
import torch

import activity_ref as ar
import f0_ref as fr
import mcd_ref as mr
from test_mcd_cpu import CFG

pytestmark = pytest.mark.gpu

HOP, W = 80, 400
EPS = 2.0 ** -24
FIELDS = ('n_cells', 'n_both_voiced', 'n_vuv_mismatch', 'vuv_error', 'f0_rmse_cents', 'f0_rmse_hz', 'logf0_corr')


def _np(t):
    return t.cpu().numpy()


def _pad(rows):
    out = np.zeros((len(rows), max(len(r) for r in rows)), np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype.is_floating_point:
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    return torch.equal(a, b)


@pytest.fixture(scope='module')
def batch():
    """Cuts of a test signal of 1, hop - 1, hop, W // 2, W // 2 + 1 and 779 samples, a row of exactly one tile of the energy
    kernel and one of a frame more, a 2 s test signal, an all-zero row and a row of 16,384 frames; the float64 energy and
    its float32 restatement of every row."""
    import _vc
    G = _vc.lib().vc_frame_energy_tile(HOP, W)
    assert G == 64
    s = fr.glide_signal(12)[0]
    rows = [s[:n] for n in (1, HOP - 1, HOP, W // 2, W // 2 + 1, 779)]
    rows += [s[:(G - 1) * HOP + 40], s[:G * HOP], fr.glide_signal(13)[0], np.zeros(1600, np.float32)]
    rows += [fr.glide_signal(15, seconds=82.0)[0][:16383 * HOP + 7]]
    lens = [len(r) for r in rows]
    assert [ar.n_frames(n, HOP) for n in lens[6:8]] == [G, G + 1] and ar.n_frames(lens[-1], HOP) == 16384
    e64 = [ar.frame_energy(r, HOP, W) for r in rows]
    e32 = [ar.frame_energy(r, HOP, W, dtype=np.float32) for r in rows]
    return dict(rows=rows, lens=lens, wav=torch.from_numpy(_pad(rows)).cuda(), e64=e64, e32=e32)


def test_energy_of_a_ragged_batch_against_the_float64_definition(batch):
    """Per row the device's worst |e - float64| may not exceed 3 x the float32 restatement's.  Where the restatement is exact
    (the all-zero row), the floor: a sum of W non-negative float32 terms carries a relative error of at most W 2^-24 of
    the row's largest energy."""
    import evaluation as ev
    r = ev.activity_batch(batch['wav'], batch['lens'])
    e = _np(r.energy).astype(np.float64)
    assert r.n_frames == [1 + n // HOP for n in batch['lens']] and e.shape == (len(batch['lens']), 16384)
    worst_dev = worst_res = 0.0
    for b, F in enumerate(r.n_frames):
        assert (e[b, F:] == 0).all(), b
        top = batch['e64'][b].max()
        dev, res = np.abs(e[b, :F] - batch['e64'][b]).max(), np.abs(batch['e32'][b].astype(np.float64) - batch['e64'][b]).max()
        rel = top if top > 0 else 1.0
        print('row %2d  %6d frames: device %.3e  float32 restatement %.3e (of the largest energy %.4g)' % (b, F, dev / rel, res / rel, top))
        assert dev <= 3.0 * (res if res > 0 else W * EPS * top), (b, dev, res)
        worst_dev, worst_res = max(worst_dev, dev / rel), max(worst_res, res / rel)
    print('worst row: device %.3e against the float32 restatement %.3e' % (worst_dev, worst_res))


def test_raw_decisions_against_float64_and_the_integer_work_exactly(batch):
    """mode 'energy', max_gap = 0: the decision of every frame equals the float64 one; no frame of these rows is marginal
    (|e / (r max) - 1| < 1e-4: a float32 sum of 400 non-negative terms and the maximum carry at most 400 x 2^-24 =
    2.4e-5 each).  Then, given the device's raw mask (and, for the voiced modes, the device's own track), smoothing,
    index, counts and intervals equal the reference exactly."""
    import evaluation as ev
    raw = ev.activity_batch(batch['wav'], batch['lens'], max_gap=0)
    hr = _np(raw.mask)
    for b, F in enumerate(raw.n_frames):
        want, marginal = ar.raw_energy(batch['e64'][b])
        assert marginal.sum() == 0, (b, int(marginal.sum()))
        assert np.array_equal(hr[b, :F] != 0, want) and (hr[b, F:] == 0).all(), b
    assert int(raw.n_active[9]) == 0 and int(raw.n_kept[9]) == raw.n_frames[9] and int(raw.n_intervals[9]) == 0      # digital silence
    f0 = ev.f0_batch(batch['wav'], batch['lens']).f0
    hf = _np(f0)
    for mode, kw in (('energy', {}), ('energy', dict(max_gap=3, min_run=4)), ('voiced', dict(max_gap=2, min_run=3)),
                     ('energy+voiced', dict(max_gap=20, min_run=10))):
        r = ev.activity_batch(batch['wav'], batch['lens'], mode=mode, f0=f0 if mode != 'energy' else None, **kw)
        _check_integer_work(r, [(hr[b, :F] != 0 if mode != 'voiced' else np.ones(F, bool)) & (hf[b, :F] > 0 if mode != 'energy' else True)
                                for b, F in enumerate(r.n_frames)], kw.get('max_gap', 20), kw.get('min_run', 0), mode)


def _check_integer_work(r, raws, max_gap, min_run, what):
    m, idx, iv = _np(r.mask), _np(r.index), _np(r.intervals)
    assert iv.shape[1] == (m.shape[1] + 1) // 2
    for b, raw in enumerate(raws):
        F = len(raw)
        want = ar.smooth(raw, max_gap, min_run)
        assert np.array_equal(m[b, :F] != 0, want) and (m[b, F:] == 0).all(), (what, b)
        c = ar.compact(want)
        assert (int(r.n_active[b]), int(r.n_kept[b]), int(r.n_intervals[b])) == (c['n_active'], c['n_kept'], len(c['intervals'])), (what, b)
        assert np.array_equal(idx[b, :c['n_kept']], c['index']) and (idx[b, c['n_kept']:] == -1).all(), (what, b)
        assert np.array_equal(iv[b, :len(c['intervals'])], c['intervals']) and (iv[b, len(c['intervals']):] == -1).all(), (what, b)


def _run_patterns(seed, lens):
    """0 / 1 rows made of runs of 1 .. 30 frames: every gap and run length near the limits of the test occurs many times."""
    rng = np.random.RandomState(seed)
    rows = []
    for n in lens:
        pieces, v = [], int(rng.randint(2))
        while sum(len(p) for p in pieces) < n:
            pieces.append(np.full(rng.randint(1, 31), v, np.float32))
            v = 1 - v
        rows.append(np.concatenate(pieces)[:n])
    return rows


def test_smoothing_and_compaction_of_patterns_up_to_16384_frames():
    """The mask launch in 'voiced' mode on 0 / 1 "tracks": rows of 1 frame to 16,384 (one frame per lane up to 1,024, then
    2 .. 16 per lane), all-active and all-inactive rows, against the reference exactly; then the AND of two rows of
    unequal length."""
    import evaluation as ev
    lens = [1, 2, 1023, 1024, 1025, 5000, 16384, 300, 300, 777]
    rows = _run_patterns(3, lens)
    rows[7][:], rows[8][:] = 1.0, 0.0
    f0 = torch.from_numpy(_pad(rows)).cuda()
    d_f, = ev._upload_lens(np.asarray(lens))
    masks = {}
    for gap, run in ((0, 0), (20, 0), (7, 12), (30, 31), (1, 2)):
        mask = ev._mask_launch(f0, f0, d_f, (2, 1e-4, gap, run))
        c = ev._compact_launch(mask, d_f)
        r = ev._ACTIVITY(mask, c.index, c.n_active, c.n_kept, c.intervals, c.n_intervals, None, lens)
        _check_integer_work(r, [x > 0 for x in rows], gap, run, (gap, run))
        masks[(gap, run)] = mask
    ma, mb = masks[(0, 0)][:, :6000].contiguous(), torch.flip(masks[(1, 2)], dims=[0])[:, :5500].contiguous()
    la, lb = [min(n, 6000) for n in lens], [min(n, 5500) for n in lens[::-1]]
    d_a, d_b = ev._upload_lens(np.asarray(la), np.asarray(lb))
    c = ev._compact_launch(ma, d_a, mb, d_b)
    ha, hb, idx = _np(ma), _np(mb), _np(c.index)
    for b in range(len(lens)):
        want = ar.compact(ha[b, :la[b]], hb[b, :lb[b]])
        assert (int(c.n_active[b]), int(c.n_kept[b]), int(c.n_intervals[b])) == (want['n_active'], want['n_kept'], len(want['intervals'])), b
        assert np.array_equal(idx[b, :want['n_kept']], want['index']) and (idx[b, want['n_kept']:] == -1).all(), b
        assert np.array_equal(_np(c.intervals)[b, :len(want['intervals'])], want['intervals']), b


def test_compact_batch_and_the_path_map_are_exact():
    import evaluation as ev
    rng = np.random.RandomState(4)
    lens = [50, 333, 1, 200]
    rows = _run_patterns(5, lens)
    rows[3][:] = 0.0                                                     # the fallback: every frame kept
    m = torch.from_numpy(_pad(rows)).cuda().to(torch.uint8)
    d_f, = ev._upload_lens(np.asarray(lens))
    c = ev._compact_launch(m, d_f)
    x = rng.standard_normal((4, 333, 7)).astype(np.float32)
    got = _np(ev.compact_batch(torch.from_numpy(x).cuda(), c.index, c.n_kept))
    idx, kept = _np(c.index), _np(c.n_kept)
    assert kept.tolist() == [ar.compact(r > 0)['n_kept'] for r in rows] and kept[3] == 200 and int(c.n_active[3]) == 0
    for b in range(4):
        assert np.array_equal(got[b, :kept[b]], x[b, idx[b, :kept[b]]]) and (got[b, kept[b]:] == 0).all(), b
    # a path over the compacted frames, a row of it shorter than the tensor, one pair with no cell
    P = 40
    path = np.full((4, P, 2), -1, np.int32)
    plen = np.array([30, 40, 1, 0], np.int32)
    for b in range(4):
        path[b, :plen[b]] = rng.randint(0, kept[b], size=(plen[b], 2))
    out = _np(ev._path_map_launch(torch.from_numpy(path).cuda(), torch.from_numpy(plen).cuda(), c.index, c.index, P))
    ident = _np(ev._path_map_launch(None, c.n_kept, c.index, c.index, 333))
    for b in range(4):
        assert np.array_equal(out[b, :plen[b]], ar.path_map(path[b, :plen[b]], idx[b], idx[b])) and (out[b, plen[b]:] == -1).all(), b
        assert np.array_equal(ident[b, :kept[b], 0], idx[b, :kept[b]]) and np.array_equal(ident[b, :, 0], ident[b, :, 1]), b
        assert (ident[b, kept[b]:] == -1).all(), b


def test_bit_identical_alone_twice_reversed_and_under_gain(batch):
    import evaluation as ev
    r = ev.activity_batch(batch['wav'], batch['lens'])
    again = ev.activity_batch(batch['wav'], batch['lens'])
    for k in ('mask', 'index', 'n_active', 'n_kept', 'intervals', 'n_intervals', 'energy'):
        assert torch.equal(getattr(r, k), getattr(again, k)), k
    for b in (0, 3, 5, 6, 7, 8):
        n = batch['lens'][b]
        one = ev.activity_batch(batch['wav'][b:b + 1, :n].contiguous(), [n])
        F = one.n_frames[0]
        assert torch.equal(one.energy[0], r.energy[b, :F]) and torch.equal(one.mask[0], r.mask[b, :F]), b
        assert torch.equal(one.index[0], r.index[b, :F]) and int(one.n_active[0]) == int(r.n_active[b]), b
    # other strides, other tile boundaries: rows reversed in a narrower batch
    sub = ev.activity_batch(torch.flip(batch['wav'][:10, :32000], dims=[0]).contiguous(), batch['lens'][:10][::-1])
    assert torch.equal(torch.flip(sub.energy, dims=[0]), r.energy[:10, :401]) and torch.equal(torch.flip(sub.mask, dims=[0]), r.mask[:10, :401])
    assert torch.equal(torch.flip(sub.n_active, dims=[0]), r.n_active[:10])
    for g in (0.5, 4.0):                                                 # a power of two scales e and its maximum alike
        s = ev.activity_batch(batch['wav'] * g, batch['lens'])
        assert torch.equal(s.energy, r.energy * (g * g)) and torch.equal(s.mask, r.mask) and torch.equal(s.index, r.index), g


def test_graph_replay_with_new_contents_and_lengths(batch):
    """Energy, mask, compaction, gather, DTW with backtrack, path map, F0 metrics and the speech-level gain with the front-end
    behind it captured on static buffers with the
    lengths in device tensors, replayed after other waveforms and other lengths were copied into the same buffers: equal
    to the eager launches.  The first call is made outside the capture."""
    import evaluation as ev
    act = ev._activity_args('energy', 40.0, 5, 0, 'test')
    wa, wb = batch['wav'][[8, 5, 7], :32000].clone(), batch['wav'][[7, 8, 8], :32000].clone()
    la = torch.tensor([32000, 779, 5120], dtype=torch.int32, device='cuda')
    lb = torch.tensor([5120, 32000, 20000], dtype=torch.int32, device='cuda')
    fa, fb = la // HOP + 1, lb // HOP + 1
    rng = np.random.RandomState(6)
    ca, cb = torch.from_numpy(rng.standard_normal((3, 401, 24)).astype(np.float32)).cuda(), torch.from_numpy(rng.standard_normal((3, 401, 24)).astype(np.float32)).cuda()
    ta, tb = torch.from_numpy(rng.uniform(-100, 300, (3, 401)).astype(np.float32)).clamp(min=0).cuda(), torch.from_numpy(rng.uniform(-100, 300, (3, 401)).astype(np.float32)).clamp(min=0).cuda()

    def launches():
        ma = ev._mask_launch(ev._energy_launch(wa, la, HOP, W), None, fa, act)
        mb = ev._mask_launch(ev._energy_launch(wb, lb, HOP, W), None, fb, act)
        ia, ib = ev._compact_launch(ma, fa), ev._compact_launch(mb, fb)
        r = ev._masked_dtw(ca, cb, ia, ib, 25.0, -1, True)
        return ma, mb, r, ia, ib, ev._f0_metrics_launch(ta, tb, fa, fb, r.path, r.path_len), ev._speech_mel(wa, la, ma, ia.n_active, CFG)

    launches()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = launches()

    def check():
        g.replay()
        torch.cuda.synchronize()
        want = launches()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
        for k in ('total', 'path_len', 'mcd', 'path'):
            assert _same(getattr(out[2], k), getattr(want[2], k)), k
        for i in (3, 4):
            for k in ('index', 'n_active', 'n_kept', 'intervals', 'n_intervals'):
                assert torch.equal(getattr(out[i], k), getattr(want[i], k)), k
        for k in FIELDS:
            assert _same(getattr(out[5], k), getattr(want[5], k)), k
        assert torch.equal(out[6], want[6])                              # the mel under the speech-level gain
        return [int(v) for v in out[3].n_active]

    first = check()
    wa.copy_(torch.flip(batch['wav'][[8, 6, 7], :32000], dims=[0]) * 0.75)
    wb.copy_(batch['wav'][[10, 10, 9], 16000:48000])
    la.copy_(torch.tensor([5040, 1, 31999], dtype=torch.int32))
    lb.copy_(torch.tensor([32000, 16000, 700], dtype=torch.int32))
    fa.copy_(la // HOP + 1)
    fb.copy_(lb // HOP + 1)
    assert check() != first


def test_no_host_synchronisation_inside_the_calls(batch):
    import evaluation as ev
    wav, lens = batch['wav'][[8, 7, 5, 8], :32000].contiguous(), [32000, 5120, 779, 20000]
    d_len, = ev._upload_lens(np.asarray(lens))
    mel = ev._mel_launch(wav, d_len, CFG)
    a = ev.activity_batch(wav, lens)
    w48 = torch.repeat_interleave(wav, 3, dim=1)
    calls = (lambda: ev.activity_batch(wav, lens),
             lambda: ev.activity_batch(wav, lens, mode='energy+voiced', min_run=3),
             lambda: ev.mcd_batch(mel, mel, a.n_frames, a.n_frames, CFG, return_path=True, mask_a=a.mask, mask_b=torch.flip(a.mask, dims=[0]) != 0),
             lambda: ev.mcd_batch(mel, mel, a.n_frames, a.n_frames, CFG, align='frame', mask_a=a.mask),
             lambda: ev.mcd_wav_batch(wav, lens, w48, [3 * n for n in lens], CFG, wav_sr_b=48000, mask='energy+voiced', return_path=True),
             lambda: ev.score_wav_batch(wav, lens, w48, [3 * n for n in lens], CFG, wav_sr_b=48000, band=100, mask='energy'),
             lambda: ev.score_wav_batch(wav, lens, wav, lens, CFG, align='frame', mask='voiced'))
    for c in calls:
        c()
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        outs = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.equal(outs[0].mask, a.mask) and torch.isfinite(outs[5].mcd).all() and int(outs[5].n_active_a[0]) == int(a.n_active[0])


def test_without_a_mask_every_result_is_what_it_was(batch):
    """mask=None and mask_a = mask_b = None take the unmasked launches: bit for bit the same fields, the new ones None."""
    import evaluation as ev
    wav, lens = batch['wav'][[8, 7], :32000].contiguous(), [32000, 5120]
    wb, lb = batch['wav'][[7, 8], :32000].contiguous(), [5120, 31000]
    s = ev.score_wav_batch(wav, lens, wb, lb, CFG)
    t = ev.score_wav_batch(wav, lens, wb, lb, CFG, mask=None, top_db=30.0, max_gap=3, min_run=2)
    m = ev.mcd_wav_batch(wav, lens, wb, lb, CFG, return_path=True)
    n = ev.mcd_wav_batch(wav, lens, wb, lb, CFG, return_path=True, mask=None)
    assert s._fields[:17] == ('mcd', 'total', 'path_len', 'path') + FIELDS + ('f0_a', 'f0_b') + ('n_active_a', 'n_active_b', 'mask_a', 'mask_b')
    for k in s._fields:
        assert _same(getattr(s, k), getattr(t, k)), k
    assert s.n_active_a is None and s.n_active_b is None and s.mask_a is None and s.mask_b is None
    for k in m._fields:
        assert _same(getattr(m, k), getattr(n, k)) and _same(getattr(m, k), getattr(s, k)), k
    d_a, d_b = ev._upload_lens(np.asarray(lens), np.asarray(lb))
    ma, mb = ev._mel_launch(wav, d_a, CFG), ev._mel_launch(wb, d_b, CFG)
    fa, fb = [1 + x // HOP for x in lens], [1 + x // HOP for x in lb]
    for kw in (dict(return_path=True), dict(align='frame')):
        p, q = ev.mcd_batch(ma, mb, fa, fb, CFG, **kw), ev.mcd_batch(ma, mb, fa, fb, CFG, mask_a=None, mask_b=None, **kw)
        for k in p._fields:
            assert _same(getattr(p, k), getattr(q, k)), k
    # masks of ones change nothing but the launches: the same path, the same figures
    ones = torch.ones((2, 401), dtype=torch.uint8, device='cuda')
    q = ev.mcd_batch(ma, mb, fa, fb, CFG, return_path=True, mask_a=ones, mask_b=ones)
    p = ev.mcd_batch(ma, mb, fa, fb, CFG, return_path=True)
    for k in p._fields:
        assert _same(getattr(p, k), getattr(q, k)), k


def test_masked_score_wav_batch_against_the_float64_pipeline():
    """A test signal against itself 2 semitones higher and 10 % slower (test_f0_gpu.py's pair), mask='energy' with
    max_gap = 5 so that the signal's 0.12 s gaps of silence stay out.  The device's masks equal the float64 reference's
    (no frame marginal); on the device's own cepstra (of the mel under the speech-level gain) and tracks the path equals mcd_ref.dtw's over the kept frames cell
    for cell after the map (test_f0_gpu.py asks the same of the unmasked path), total is within the derived float32
    bound of test_mcd_gpu.py, 2 (Fa + Fb + 26) 2^-24 with the kept counts, the counts are exact and the F0 figures within
    3 x the float32 restatement's error (and the spacing of float32)."""
    import evaluation as ev
    a, _, _ = fr.glide_signal(21, seconds=2.0)
    b, _, _ = fr.glide_signal(21, seconds=2.0, pitch=2.0 ** (2.0 / 12.0), stretch=1.1)
    c, _, _ = fr.glide_signal(22, seconds=1.5)
    wa, la = _pad([a, c]), [len(a), len(c)]
    wb, lb = _pad([b, a]), [len(b), len(a)]
    s = ev.score_wav_batch(wa, la, wb, lb, CFG, mask='energy', max_gap=5)
    m = ev.mcd_wav_batch(wa, la, wb, lb, CFG, return_path=True, mask='energy', max_gap=5)
    for k in ('mcd', 'total', 'path_len', 'path'):
        assert torch.equal(getattr(s, k), getattr(m, k)), k
    scale = mr.default_scale(CFG['M_dB_norm_factor'])
    for p, (xa, xb) in enumerate(((a, b), (c, a))):
        Fa, Fb = 1 + len(xa) // HOP, 1 + len(xb) // HOP
        masks = []
        for x, dev in ((xa, _np(s.mask_a[p])), (xb, _np(s.mask_b[p]))):
            ref = ar.activity(x, HOP, W, max_gap=5)
            assert ref['marginal'].sum() == 0 and np.array_equal(dev[:len(ref['mask'])] != 0, ref['mask'])
            assert 0 < ref['n_active'] < len(ref['mask'])                # the mask does something
            masks.append(ref['mask'])
        assert (int(s.n_active_a[p]), int(s.n_active_b[p])) == (int(masks[0].sum()), int(masks[1].sum()))
        d_la, d_lb = ev._upload_lens(np.array([len(xa)]), np.array([len(xb)]))
        cep = []
        for x, d_l, F, dm, dn in ((xa, d_la, Fa, s.mask_a, s.n_active_a), (xb, d_lb, Fb, s.mask_b, s.n_active_b)):
            mel = ev._speech_mel(torch.from_numpy(x).cuda().view(1, -1), d_l, dm[p:p + 1, :F].contiguous(), dn[p:p + 1].contiguous(), CFG)
            cep.append(_np(ev.mel_cepstra(mel))[0, :F].astype(np.float64))
        ca, cb = cep
        fa, fb = _np(s.f0_a[p])[:Fa], _np(s.f0_b[p])[:Fb]
        want = ar.masked_pipeline(ca, cb, masks[0], masks[1], fa, fb, scale)
        n = int(s.path_len[p])
        path = _np(s.path[p])
        assert n == want['path_len'] and np.array_equal(path[:n], want['path']) and (path[n:] == -1).all(), p
        assert masks[0][path[:n, 0]].all() and masks[1][path[:n, 1]].all()
        err, bound = abs(float(s.total[p]) - want['total']) / want['total'], 2.0 * (masks[0].sum() + masks[1].sum() + 26) * EPS
        print('pair %d: masked MCD %.4f dB over %d cells (float64 %.4f), total rel err %.3e (bound %.3e); %d / %d and %d / %d frames active'
              % (p, float(s.mcd[p]), n, want['mcd'], err, bound, masks[0].sum(), Fa, masks[1].sum(), Fb))
        assert err <= bound
        rest = fr.metrics(fa, fb, Fa, Fb, want['path'], dtype=np.float32)
        for k in FIELDS[:3]:
            assert int(getattr(s, k)[p]) == want['metrics'][k], (p, k)
        for k in FIELDS[3:]:
            v, w64 = float(getattr(s, k)[p]), want['metrics'][k]
            if np.isnan(w64):
                assert np.isnan(v), (p, k)
                continue
            yard = abs(float(rest[k]) - w64)
            print('pair %d %-14s device %.6f  float64 %.6f  err %.3e  float32 restatement %.3e' % (p, k, v, w64, abs(v - w64), yard))
            assert abs(v - w64) <= 3.0 * max(yard, float(np.spacing(np.float32(abs(w64))))), (p, k)


def test_speech_gain_against_float64_and_the_scaled_rows(batch):
    """The gain of every row of the ragged batch under its own default mask against activity_ref.speech_gain.  The device
    adds |x| in float64 (at most 2^21 terms here: a relative error below 2^-32) and rounds the quotient to float32 once:
    the bound is one float32 rounding, 2^-24 relative, doubled for the float32 target.  The scaled rows are gain * x exactly,
    zeros beyond the length."""
    import evaluation as ev
    r = ev.activity_batch(batch['wav'], batch['lens'])
    d_len, = ev._upload_lens(np.asarray(batch['lens']))
    B, Lmax = batch['wav'].shape
    gain = torch.empty((B,), dtype=torch.float32, device='cuda')
    lib, st = ev._vc.lib(), ev._vc.current_stream()
    ev._vc.check(lib.vc_speech_gain_f32(ev._vc.ptr(batch['wav']), ev._vc.ptr(d_len), B, Lmax, Lmax, HOP, ev._vc.ptr(r.mask), ev._vc.ptr(r.n_active),
                                        r.mask.shape[1], 0.003, ev._vc.ptr(gain), st))
    out = torch.empty_like(batch['wav'])
    ev._vc.check(lib.vc_scale_rows_f32(ev._vc.ptr(batch['wav']), ev._vc.ptr(d_len), B, Lmax, Lmax, ev._vc.ptr(gain), ev._vc.ptr(out), st))
    g, hm = _np(gain).astype(np.float64), _np(r.mask)
    for b, n in enumerate(batch['lens']):
        want = ar.speech_gain(batch['rows'][b], hm[b, :r.n_frames[b]], HOP, float(np.float32(0.003)))
        print('row %2d: gain %.6g, float64 %.6g, rel err %.2e' % (b, g[b], want, abs(g[b] / want - 1)))
        assert abs(g[b] / want - 1) <= 2.0 * EPS, (b, g[b], want)
    assert g[9] == 1.0                                                    # the all-zero row
    assert torch.equal(out, batch['wav'] * gain[:, None])


@pytest.fixture(scope='module')
def silence_scores():
    import evaluation as ev
    a, b, edits = ar.silence_pair(31)
    masked = ev.score_wav_batch(a[None], [len(a)], b[None], [len(b)], CFG, mask='energy')
    plain = ev.score_wav_batch(a[None], [len(a)], b[None], [len(b)], CFG)
    return a, b, edits, masked, plain


def test_an_utterance_against_its_copy_with_silence_added_the_path_stays_on_speech(silence_scores):
    """activity_ref.silence_pair: 2 s of a broadband test signal against its copy with 0.5 s of leading "silence" (white noise
    60 dB below the peak), a 0.3 s pause cut in and 2 s of trailing silence.  With mask='energy' every path cell lies on
    frames active on both sides, the masks are the float64 reference's, and n_active_b is within 4 ceil(W / hop) = 20
    frames of n_active_a: the pieces are whole hops, so a frame of b reads what its frame of a reads unless its window of
    W samples straddles one of the four places where speech and silence meet, and ceil(W / hop) = 5 consecutive frames
    straddle a place.  (Float64 on the CPU: 401 and 410 active frames.)"""
    a, b, edits, s, _ = silence_scores
    A, B = ar.activity(a, HOP, W), ar.activity(b, HOP, W)
    assert A['marginal'].sum() == 0 and B['marginal'].sum() == 0
    ma, mb = _np(s.mask_a[0]) != 0, _np(s.mask_b[0]) != 0
    assert np.array_equal(ma[:len(A['mask'])], A['mask']) and np.array_equal(mb[:len(B['mask'])], B['mask'])
    n = int(s.path_len[0])
    path = _np(s.path[0])[:n]
    assert n >= max(int(s.n_active_a[0]), int(s.n_active_b[0])) and ma[path[:, 0]].all() and mb[path[:, 1]].all()
    na, nb = int(s.n_active_a[0]), int(s.n_active_b[0])
    print('active frames: %d of %d and %d of %d; intervals of b: %s' % (na, len(A['mask']), nb, len(B['mask']), B['intervals'].tolist()))
    assert abs(nb - na) <= 4 * -(-W // HOP)
    # the leading and trailing silence and the pause are out: two intervals, from the first edit to the last
    assert len(B['intervals']) == 2 and abs(B['intervals'][0][0] - edits[0] // HOP) <= 3 and abs(B['intervals'][1][1] - edits[3] // HOP) <= 3
    assert int(s.n_cells[0]) == n


def test_an_utterance_against_its_copy_with_silence_added_the_masked_mcd_is_lower(silence_scores):
    """The masked MCD of that pair must lie strictly below the unmasked MCD of the same pair.

    The float64 pipeline on the CPU (the front-end oracle on gain * x with its normalisation off, activity_ref.speech_gain,
    mcd_ref.dtw): 0.374 dB masked over 410 cells, 3.976 dB unmasked over 961 cells.  With the front-end's own
    normalisation over the whole waveform the masked figure is 8.764 dB over 411 cells: the copy, 58 % silence, is
    amplified 2.4 times more than the utterance, and the front-end floors the mel power, so its cells rise 15 dB against
    a fixed floor -- which is why the masked scores take the gain over the speech samples (include/vc_hip.h)."""
    _, _, _, s, plain = silence_scores
    print('MCD of the pair: masked %.4f dB over %d cells, unmasked %.4f dB over %d cells'
          % (float(s.mcd[0]), int(s.path_len[0]), float(plain.mcd[0]), int(plain.path_len[0])))
    assert float(s.mcd[0]) < float(plain.mcd[0])
