"""The pitch tracker and the F0 / voicing figures on the device against tests/f0_ref.py: a ragged batch from one sample to
60 s against the float64 definition (voicing equal off the threshold, errors against the float32 restatement's), the four
bit-identities (alone / batched, twice, gain, graph replay), the figures along the DTW path of mcd_batch and without a
path, score_wav_batch against mcd_wav_batch and against the float64 pipeline, and no host synchronisation."""
import numpy as np
import pytest
import torch

import f0_ref as fr
import mcd_ref as mr
from test_mcd_cpu import CFG

pytestmark = pytest.mark.gpu

HOP, W = 80, 512
TAU_MIN, TAU_MAX = fr.lag_range(16000)
FIELDS = ('n_cells', 'n_both_voiced', 'n_vuv_mismatch', 'vuv_error', 'f0_rmse_cents', 'f0_rmse_hz', 'logf0_corr')


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """Bit-identical, NaN equal to NaN."""
    if a.dtype.is_floating_point:
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    return torch.equal(a, b)


def _pad(rows):
    out = np.zeros((len(rows), max(len(r) for r in rows)), np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


@pytest.fixture(scope='module')
def batch():
    """The four 2 s test signals, cuts of one of them from 1 sample (shorter than a frame span of 780) up, a 60 s signal,
    an all-zero row and a row of white noise; the float64 definition and the float32 restatement of every row."""
    rng = np.random.RandomState(5)
    rows = [fr.glide_signal(s)[0] for s in (11, 12, 13, 14)]
    rows += [rows[1][:n] for n in (1, 79, 300, 779, 5001)]
    rows += [fr.glide_signal(15, seconds=60.0)[0], np.zeros(16000, np.float32), (0.1 * rng.standard_normal(16000)).astype(np.float32)]
    lens = [len(r) for r in rows]
    ref = [fr.yin(r, details=True) for r in rows]
    res = [fr.yin(r, dtype=np.float32) for r in rows]
    return dict(rows=rows, lens=lens, wav=torch.from_numpy(_pad(rows)).cuda(), ref=ref, res=res)


def test_a_ragged_batch_against_the_float64_definition(batch):
    """Voicing equals the float64 decision on every frame that is not marginal (f0_ref.yin: the decision or the chosen
    dip changes when the threshold moves by 1e-3); at most 1 % of the frames may be marginal, of the batch and of
    every row of 100 frames or more, and none of a shorter row.  On frames voiced on both
    sides the device's worst F0 error (cents) and aperiodicity error against float64 may not exceed 3 x the float32
    restatement's on the same frames.

    Where the restatement's error is zero, the floor: every d(tau) and every running sum is a sum of at most
    W + tau_max non-negative float32 terms, so d' carries a relative error of at most delta = (W + tau_max) 2^-24 =
    4.6e-5.  The aperiodicity is one d': floor delta * d'.  The parabola's offset 0.5 (y0 - y2) / (y0 - 2 y1 + y2) moves
    by at most delta * max(y) * (1 + 4 |offset|) / denominator (numerator error 2 delta max(y) / 2, denominator error
    4 delta max(y) times |offset| / denominator), and F0 by (1200 / ln 2) * that / (tau + offset) cents."""
    import evaluation as ev
    r = ev.f0_batch(batch['wav'], batch['lens'])
    f0, ap = _np(r.f0), _np(r.aperiodicity)
    assert r.n_frames == [1 + n // HOP for n in batch['lens']] and f0.shape == (len(batch['lens']), 1 + batch['wav'].shape[1] // HOP)
    n_all = n_marg = 0
    worst = dict(dev_c=0.0, res_c=0.0, dev_a=0.0, res_a=0.0)
    for b, F in enumerate(r.n_frames):
        f64, a64, det = batch['ref'][b]
        f32, a32 = batch['res'][b]
        assert (f0[b, F:] == 0).all() and (ap[b, F:] == 1).all(), b
        keep = ~det['marginal']
        n_all, n_marg = n_all + F, n_marg + int(det['marginal'].sum())
        assert det['marginal'].sum() <= (0.01 * F if F >= 100 else 0), (b, F, int(det['marginal'].sum()))      # the cap, row by row
        assert np.array_equal(f0[b, :F][keep] > 0, f64[keep] > 0), (b, np.nonzero((f0[b, :F] > 0) != (f64 > 0))[0][:10])
        both = keep & (f64 > 0) & (f32 > 0) & (f0[b, :F] > 0)
        e_a, y_a = np.abs(ap[b, :F].astype(np.float64) - a64), np.abs(a32.astype(np.float64) - a64)
        e_c = np.abs(fr.cents(f0[b, :F][both], f64[both])) if both.any() else np.zeros(1)
        y_c = np.abs(fr.cents(f32[both], f64[both])) if both.any() else np.zeros(1)
        fl_c = det['floor_cents'][both].max() if both.any() else 0.0
        print('row %2d  %6d frames, %5d voiced, %d marginal: F0 device %.3e cents, restatement %.3e;  aperiodicity device %.3e, '
              'restatement %.3e' % (b, F, int(both.sum()), int(det['marginal'].sum()), e_c.max(), y_c.max(), e_a[keep].max(), y_a[keep].max()))
        assert e_c.max() <= 3.0 * (y_c.max() if y_c.max() > 0 else fl_c), (b, e_c.max(), y_c.max(), fl_c)
        ya = y_a[keep].max() if keep.any() else 0.0
        assert (e_a[keep].max() if keep.any() else 0.0) <= 3.0 * (ya if ya > 0 else det['floor_ap'][keep].max() if keep.any() else 0.0), b
        worst = dict(dev_c=max(worst['dev_c'], e_c.max()), res_c=max(worst['res_c'], y_c.max()),
                     dev_a=max(worst['dev_a'], e_a[keep].max() if keep.any() else 0.0), res_a=max(worst['res_a'], ya))
    print('all rows: %d frames, %d marginal;  F0 device %.3e cents against restatement %.3e;  aperiodicity device %.3e against %.3e'
          % (n_all, n_marg, worst['dev_c'], worst['res_c'], worst['dev_a'], worst['res_a']))
    assert n_marg <= 0.01 * n_all
    # silence: exactly unvoiced with aperiodicity one; noise: unvoiced throughout
    z = len(batch['lens']) - 2
    assert (f0[z] == 0).all() and (ap[z] == 1).all()
    assert (f0[z + 1, :201] == 0).mean() > 0.95


def test_bit_identical_alone_twice_and_under_gain(batch):
    import evaluation as ev
    r = ev.f0_batch(batch['wav'], batch['lens'])
    again = ev.f0_batch(batch['wav'], batch['lens'])
    assert torch.equal(r.f0, again.f0) and torch.equal(r.aperiodicity, again.aperiodicity)
    for b in (0, 4, 6, 8, 9):
        n = batch['lens'][b]
        one = ev.f0_batch(batch['wav'][b:b + 1, :n].contiguous(), [n])
        F = one.n_frames[0]
        assert torch.equal(one.f0[0], r.f0[b, :F]) and torch.equal(one.aperiodicity[0], r.aperiodicity[b, :F]), b
    # other strides of the same rows, other tile boundaries: rows reversed in a narrower batch
    sub = ev.f0_batch(torch.flip(batch['wav'][:9, :32000], dims=[0]).contiguous(), batch['lens'][:9][::-1])
    assert torch.equal(torch.flip(sub.f0, dims=[0]), r.f0[:9, :401])
    for g in (0.5, 4.0):
        s = ev.f0_batch(batch['wav'] * g, batch['lens'])
        assert torch.equal(s.f0, r.f0) and torch.equal(s.aperiodicity, r.aperiodicity), g


def test_graph_replay_with_new_contents_and_lengths(batch):
    """The F0 launches of both sides and the metrics launch captured on static buffers with the lengths in device
    tensors, replayed after other waveforms and other lengths were copied into the same buffers: equal to the eager
    public calls.  The first call is made outside the capture."""
    import evaluation as ev
    args = ev._f0_args(16000, HOP, W, 60.0, 400.0, 0.15, 'test')
    wa, wb = batch['wav'][0:3, :32000].clone(), batch['wav'][1:4, :32000].clone()
    la = torch.tensor([32000, 32000, 32000], dtype=torch.int32, device='cuda')
    lb, fa, fb = la.clone(), la // HOP + 1, la // HOP + 1

    def launches():
        ta, tb = ev._f0_launch(wa, la, args), ev._f0_launch(wb, lb, args)
        return ta, tb, ev._f0_metrics_launch(ta[0], tb[0], fa, fb, None, None)

    launches()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ta, tb, m = launches()

    def check(len_a, len_b):
        g.replay()
        torch.cuda.synchronize()
        ea, eb = ev.f0_batch(wa, len_a), ev.f0_batch(wb, len_b)
        assert torch.equal(ta[0], ea.f0) and torch.equal(ta[1], ea.aperiodicity) and torch.equal(tb[0], eb.f0)
        want = ev.f0_metrics_batch(ea.f0, eb.f0, ea.n_frames, eb.n_frames)
        for k in FIELDS:
            assert _same(getattr(m, k), getattr(want, k)), k

    check([32000] * 3, [32000] * 3)
    wa.copy_(torch.flip(batch['wav'][0:3, :32000], dims=[0]) * 0.75)
    wb.copy_(batch['wav'][9:12, 16000:48000])
    new_a, new_b = [20000, 1, 31999], [32000, 16000, 700]
    for d, h in ((la, new_a), (lb, new_b)):
        d.copy_(torch.tensor(h, dtype=torch.int32))
    fa.copy_(la // HOP + 1)
    fb.copy_(lb // HOP + 1)
    check(new_a, new_b)


def _bound(want, yard):
    """The project's rule for a scalar figure: 3 x the float32 restatement's error, and not below the spacing of float32
    at the value (the device rounds its float64 result to float32 once)."""
    return 3.0 * max(yard, float(np.spacing(np.float32(abs(want)))))


def _check_metrics(got, b, fa, fb, la, lb, path, what):
    want, rest = fr.metrics(fa, fb, la, lb, path), fr.metrics(fa, fb, la, lb, path, dtype=np.float32)
    for k in FIELDS[:3]:
        assert int(getattr(got, k)[b]) == want[k], (what, b, k, int(getattr(got, k)[b]), want[k])
    for k in FIELDS[3:]:
        v = float(getattr(got, k)[b])
        if np.isnan(want[k]):
            assert np.isnan(v), (what, b, k, v)
            continue
        err, yard = abs(v - want[k]), abs(float(rest[k]) - want[k])
        print('%s pair %d %-14s device %.6f  float64 %.6f  err %.3e  float32 restatement %.3e' % (what, b, k, v, want[k], err, yard))
        assert err <= _bound(want[k], yard), (what, b, k, err, yard)
    return want


def _mel(wav, lens):
    import evaluation as ev
    d_len, = ev._upload_lens(np.asarray(lens))
    return ev._mel_launch(wav, d_len, CFG)


def test_metrics_along_the_dtw_path_and_without_a_path(batch):
    """Pairs of the batch's rows (other fundamentals, other gaps, a short cut, the silent and the noisy row) through the
    front-end and mcd_batch(return_path=True); the figures along that path and frame by frame against the float64
    figures on the device's own f0 and path.  The counts are exact."""
    import evaluation as ev
    ia, ib = [0, 1, 2, 8, 10, 3, 11], [1, 2, 3, 1, 0, 10, 11]
    wav = batch['wav'][:, :32000]
    wa, wb = wav[ia].contiguous(), wav[ib].contiguous()
    la, lb = [min(batch['lens'][i], 32000) for i in ia], [min(batch['lens'][i], 32000) for i in ib]
    ta, tb = ev.f0_batch(wa, la), ev.f0_batch(wb, lb)
    res = ev.mcd_batch(_mel(wa, la), _mel(wb, lb), ta.n_frames, tb.n_frames, CFG, return_path=True)
    got = ev.f0_metrics_batch(ta.f0, tb.f0, ta.n_frames, tb.n_frames, res.path, res.path_len)
    flat = ev.f0_metrics_batch(ta.f0, tb.f0, ta.n_frames, tb.n_frames)
    ha, hb, hp, hn = _np(ta.f0), _np(tb.f0), _np(res.path), _np(res.path_len)
    for b in range(len(ia)):
        w = _check_metrics(got, b, ha[b], hb[b], ta.n_frames[b], tb.n_frames[b], hp[b, :hn[b]], 'path')
        assert w['n_cells'] == hn[b]
        # the rows of -1 beyond the path's end change nothing
        assert fr.metrics(ha[b], hb[b], ta.n_frames[b], tb.n_frames[b], hp[b])['n_cells'] == w['n_cells']
        _check_metrics(flat, b, ha[b], hb[b], ta.n_frames[b], tb.n_frames[b], None, 'flat')
    assert np.isnan(_np(got.f0_rmse_cents)[4]) and int(got.n_both_voiced[4]) == 0             # the silent row has no voiced frame


def _score_against_the_pipeline(s, b, xa, xb, what):
    """score_wav_batch's figures of pair b against the float64 pipeline on the device's own mel (cepstra) and waveforms
    xa, xb at 16 kHz: mcd_ref.dtw's path, f0_ref.yin, f0_ref.metrics.

    Bound.  With the same cells and the same voicing, an RMSE moves by at most the largest change of a cell's value: two
    tracks, each within 3 x the float32 restatement's worst F0 error of the float64 track (the rule of the first test),
    so |rmse - reference| <= 6 x that error, plus the rounding of the float32 result.  A frame whose decision is marginal
    is set aside as there: it takes the device's value on both sides of the comparison.  The cells are those of
    mcd_ref.dtw's float64 path on the device's own cepstra; the device's path must be that path, cell for cell.  (A
    float32 and a float64 recurrence can part at a near-tie in the minimum of three: should this assertion ever fail on
    other signals with a handful of differing cells and the DTW tests green, look for such a tie before suspecting the
    kernel.)"""
    import evaluation as ev
    la, lb = len(xa), len(xb)
    Fa, Fb = 1 + la // HOP, 1 + lb // HOP
    refs, yard = [], 0.0
    for x, dev in ((xa, _np(s.f0_a[b])), (xb, _np(s.f0_b[b]))):
        f64, _, det = fr.yin(x, details=True)
        f32, _ = fr.yin(x, dtype=np.float32)
        F = len(f64)
        keep = ~det['marginal']
        assert np.array_equal(dev[:F][keep] > 0, f64[keep] > 0)
        both = keep & (f64 > 0) & (f32 > 0)
        yard = max(yard, np.abs(fr.cents(f32[both], f64[both])).max())
        f64[~keep] = dev[:F][~keep]
        refs.append(f64)
    d_la, d_lb = ev._upload_lens(np.array([la]), np.array([lb]))
    ca = _np(ev.mel_cepstra(ev._mel_launch(torch.from_numpy(xa).cuda().view(1, -1), d_la, CFG)))[0, :Fa].astype(np.float64)
    cb = _np(ev.mel_cepstra(ev._mel_launch(torch.from_numpy(xb).cuda().view(1, -1), d_lb, CFG)))[0, :Fb].astype(np.float64)
    p64 = mr.dtw(ca, cb, mr.default_scale(CFG['M_dB_norm_factor']))[2]
    n = int(s.path_len[b])
    path = _np(s.path[b])[:n]
    differ = -1 if len(p64) != n else int((p64 != path).any(axis=1).sum())
    assert differ == 0, '%s: the device path (%d cells) is not mcd_ref.dtw\'s float64 path (%d cells; %d differ)' % (what, n, len(p64), differ)
    want = fr.metrics(refs[0], refs[1], Fa, Fb, p64)
    got = {k: float(getattr(s, k)[b]) for k in FIELDS}
    tol_c = 6.0 * yard + float(np.spacing(np.float32(want['f0_rmse_cents'])))
    print('%s: device vuv_error %.4f  f0_rmse_cents %.4f  f0_rmse_hz %.3f  logf0_corr %.5f over %d cells, %d both voiced'
          % (what, got['vuv_error'], got['f0_rmse_cents'], got['f0_rmse_hz'], got['logf0_corr'], n, int(got['n_both_voiced'])))
    print('%s: float64 pipeline (mcd_ref.dtw path, equal to the device path; f0_ref): vuv_error %.4f  f0_rmse_cents %.4f (difference '
          '%.3e, bound %.3e)' % (what, want['vuv_error'], want['f0_rmse_cents'], abs(got['f0_rmse_cents'] - want['f0_rmse_cents']), tol_c))
    assert [int(got[k]) for k in FIELDS[:3]] == [want[k] for k in FIELDS[:3]]
    assert got['vuv_error'] == np.float32(want['vuv_error'])
    assert abs(got['f0_rmse_cents'] - want['f0_rmse_cents']) <= tol_c
    return got, want


def test_score_wav_batch(batch):
    import audio_lib
    import evaluation as ev
    # 1. the MCD side is mcd_wav_batch's, bit for bit
    a, _, _ = fr.glide_signal(21, seconds=2.0)
    b, _, _ = fr.glide_signal(21, seconds=2.0, pitch=2.0 ** (2.0 / 12.0), stretch=1.1)
    c, _, _ = fr.glide_signal(22, seconds=1.5)
    wa, la = _pad([a, c]), [len(a), len(c)]
    wb, lb = _pad([b, a]), [len(b), len(a)]
    s = ev.score_wav_batch(wa, la, wb, lb, CFG)
    m = ev.mcd_wav_batch(wa, la, wb, lb, CFG, return_path=True)
    for k in ('mcd', 'total', 'path_len', 'path'):
        assert torch.equal(getattr(s, k), getattr(m, k)), k
    f = ev.score_wav_batch(wa, la, wb, lb, CFG, align='frame')
    assert torch.equal(f.mcd, ev.mcd_wav_batch(wa, la, wb, lb, CFG, align='frame').mcd) and f.path is None and f.total is None
    assert _np(f.n_cells).tolist() == [min(1 + x // HOP, 1 + y // HOP) for x, y in zip(la, lb)]
    assert torch.equal(s.f0_a, ev.f0_batch(wa, la).f0) and torch.equal(s.f0_b, ev.f0_batch(wb, lb).f0)
    # 2. the same utterance 2 semitones higher and 10 % slower: about 200 cents (reported; asserted against the pipeline)
    _score_against_the_pipeline(s, 0, a, b, '2 semitones up, 10 % slower')
    # 3. an utterance against its own 48 kHz copy: side b goes 16 -> 48 -> 16 kHz on the device
    up, n_up = audio_lib.resample_batch(torch.from_numpy(a).cuda().view(1, -1), None, sr_in=16000, sr_out=48000)
    back, n_back = audio_lib.resample_batch(up, None, sr_in=48000, sr_out=16000)
    assert list(n_back) == [len(a)]
    s48 = ev.score_wav_batch(a[None], [len(a)], up, [3 * len(a)], CFG, wav_sr_b=48000)
    m48 = ev.mcd_wav_batch(a[None], [len(a)], up, [3 * len(a)], CFG, wav_sr_b=48000, return_path=True)
    assert torch.equal(s48.mcd, m48.mcd) and torch.equal(s48.path, m48.path)
    _score_against_the_pipeline(s48, 0, a, _np(back)[0], '16 kHz against its own 48 kHz copy')


def test_no_host_synchronisation_inside_the_calls(batch):
    import evaluation as ev
    wav, lens = batch['wav'][:4, :32000].contiguous(), [32000, 20000, 801, 32000]
    t = ev.f0_batch(wav, lens)
    mel = _mel(wav, lens)
    res = ev.mcd_batch(mel, mel, t.n_frames, t.n_frames[::-1], CFG, return_path=True)
    w48 = torch.repeat_interleave(wav, 3, dim=1)
    calls = (lambda: ev.f0_batch(wav, lens),
             lambda: ev.f0_metrics_batch(t.f0, t.f0, t.n_frames, t.n_frames[::-1], res.path, res.path_len),
             lambda: ev.f0_metrics_batch(t.f0, t.f0, t.n_frames, t.n_frames[::-1]),
             lambda: ev.score_wav_batch(wav, lens, w48, [3 * n for n in lens], CFG, wav_sr_b=48000, band=100))
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
    assert torch.isfinite(outs[0].f0).all() and int(outs[1].n_cells[0]) == int(res.path_len[0])
