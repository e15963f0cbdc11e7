"""The pitch tracker with several candidates per frame on the device against tests/f0_track_ref.py: the Viterbi launch
alone, exact on lattices whose sums are exact in float32; the candidate launch alone on a ragged batch from one sample
to 60 s against the float64 definition; the two chained (YIN's voicing with zero transition costs, the float64 path on
the device's own lattice, the octave errors of the weak fundamental); the bit-identities (alone / batched, twice, rows
reversed, graph replay); no host synchronisation; score_wav_batch(f0_method='viterbi')."""
import math

import numpy as np
import pytest
import torch

import f0_ref as fr
import f0_track_ref as tr
from test_mcd_cpu import CFG

pytestmark = pytest.mark.gpu

HOP, W = 80, 512
TAU_MIN, TAU_MAX = fr.lag_range(16000)
DELTA = (W + TAU_MAX) * 2.0 ** -24
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


# ------------------------------------------------------------------------------------------------- the Viterbi launch alone
@pytest.mark.parametrize('n_cand,empty_row', [(1, 0), (8, 3), (15, 5)])
def test_viterbi_is_exact_on_dyadic_lattices(n_cand, empty_row):
    """Costs and pitches multiples of 1/64 in [0, 2], the three parameters multiples of 1/16: every float32 sum is exact
    (f0_track_ref.dyadic_lattice), so state and total must equal the float64 reference exactly.  Seven rows of 1, 2, 3
    and T - 1, T, T + 1 frames (T: the kernel's staging tile) and 4,097; the last row's length is given as 5,000 and
    clamped by the kernel; one row has n = 0 in every frame.  Slots beyond n hold cost 0: reading one would win."""
    import _vc
    import evaluation as ev
    T = _vc.lib().vc_f0_viterbi_tile()
    frames = [1, 2, 3, T - 1, T, T + 1, 4097]
    rng = np.random.RandomState(7 + n_cand)
    Fmax = 4097
    pitch, cost = np.zeros((7, Fmax, n_cand), np.float32), np.zeros((7, Fmax, n_cand), np.float32)
    n = np.zeros((7, Fmax), np.int32)
    for b in range(7):
        pitch[b], cost[b], n[b] = tr.dyadic_lattice(rng, Fmax, n_cand)          # also beyond the row's frames: not to be read
    n[empty_row] = 0
    uc, jc, sc = (rng.randint(1, 33, 3) / 16.0).tolist()
    cand_f0 = (2.0 ** (pitch.astype(np.float64) + 6.0)).astype(np.float32)
    d = [torch.from_numpy(a).cuda() for a in (pitch, cost, n, cand_f0)]
    given = torch.tensor(frames[:6] + [5000], dtype=torch.int32, device='cuda')
    state, total, f0 = ev._f0_viterbi_launch(d[0], d[1], d[2], given, (uc, jc, sc), d[3])
    pub = ev.f0_viterbi_batch(pitch, cost, n, frames, uc, jc, sc, f0=cand_f0)      # the public call, lengths as given
    assert torch.equal(pub.state, state) and torch.equal(pub.total, total) and torch.equal(pub.f0, f0)
    none = ev.f0_viterbi_batch(d[0], d[1], d[2], frames, uc, jc, sc)
    assert none.f0 is None and torch.equal(none.state, state) and torch.equal(none.total, total)
    state, total, f0 = _np(state), _np(total), _np(f0)
    for b, F in enumerate(frames):
        want, tot = tr.viterbi(pitch[b, :F], cost[b, :F], n[b, :F], uc, jc, sc)
        assert np.array_equal(state[b, :F], want), (b, F, np.nonzero(state[b, :F] != want)[0][:8])
        assert total[b] == np.float32(tot) and float(np.float32(tot)) == tot, (b, total[b], tot)
        assert (state[b, F:] == -1).all() and (f0[b, F:] == 0).all()
        assert np.array_equal(f0[b, :F], np.where(want > 0, cand_f0[b, np.arange(F), np.maximum(want, 1) - 1], 0))
        assert (want <= n[b, :F]).all()
    assert (state[empty_row, :frames[empty_row]] == 0).all()


# ------------------------------------------------------------------------------------------------------- the ragged batch
@pytest.fixture(scope='module')
def batch():
    """test_f0_gpu.py's ragged batch (the four 2 s signals, cuts of one of them from 1 sample up, 60 s, an all-zero row,
    white noise) and the weak-fundamental seeds 0 and 1; d' of every row in float64 and in the float32 restatement,
    computed once."""
    rng = np.random.RandomState(5)
    rows = [fr.glide_signal(s)[0] for s in (11, 12, 13, 14)]
    rows += [rows[1][:n] for n in (1, 79, 300, 779, 5001)]
    rows += [fr.glide_signal(15, seconds=60.0)[0], np.zeros(16000, np.float32), (0.1 * rng.standard_normal(16000)).astype(np.float32)]
    weak = [tr.weak_signal(s) for s in (0, 1)]
    rows += [w[0] for w in weak]
    lens = [len(r) for r in rows]
    return dict(rows=rows, lens=lens, wav=torch.from_numpy(_pad(rows)).cuda(), weak={12: weak[0], 13: weak[1]}, silent=10,
                dp64=[tr.dprime(r) for r in rows], dp32=[tr.dprime(r, dtype=np.float32) for r in rows])


def _floor_cents(row, tau):
    """What a relative error of DELTA in every d' can move F0 by at lag tau, in cents (test_f0_gpu.py's floor)."""
    y0, y1, y2 = (float(v) for v in row[tau - 1:tau + 2])
    den = y0 - 2 * y1 + y2
    if den <= 0:
        return 0.0
    off = min(max(0.5 * (y0 - y2) / den, -0.5), 0.5)
    return 1200.0 / math.log(2.0) * DELTA * max(y0, y1, y2) * (1 + 4 * abs(off)) / den / (tau + off)


@pytest.mark.parametrize('n_cand,ceiling,row_cap', [(8, 0.3, True), (8, 1.0, False), (3, 0.3, True), (15, 1.0, False)])
def test_candidates_of_a_ragged_batch_against_the_float64_definition(batch, n_cand, ceiling, row_cap):
    """aperiodicity is f0_batch's bit for bit.  Lags and n equal the float64 reference on every frame that is not marginal
    (f0_track_ref.marginal_frames: a local-minimum flag, the ceiling or rank n_cand against n_cand + 1 changes under a
    relative move of (W + tau_max) 2^-24 in d').  A device lag is read from its f0: the period sr / f0 lies within half a
    sample of it.  On agreeing candidates the worst error of f0 (cents) and of cost against float64 is at most 3 x the
    float32 restatement's own, row by row (where that is zero: the floor of test_f0_gpu.py).  pitch is log2 of the
    device's own f0 within two spacings of float32 at 8 (log2f is within one).

    Marginal frames are capped at 1 % of the batch, and with row_cap at 1 % of every row of 100 frames or more and none
    in a shorter row.  The reference alone decides which frames are marginal, and at ceiling = 1 it cannot meet the caps
    row by row on these inputs: two neighbouring lags at the flat bottom of a shallow dip (d' of 0.5 to 0.9) are often
    within 2 x 4.6e-5 of each other, and the one-sample row has d' = 1 + rounding noise at every lag, so with n_cand = 8
    it sets aside 9 of 401 frames of the second glide (2.2 %), 9 of 201 of the noise row (4.5 %), 7 and 8 of 401 of the
    weak-fundamental rows and the only frame of the one-sample row -- 51 of 14,888 in all (0.34 %), while its own float32
    restatement differs from it on 2 frames.  At ceiling = 0.3 every row is within the caps (at most 1 of 401; none in a
    short row) and the restatement differs on none.  So the row caps are asserted at ceiling 0.3 and the batch cap at
    both; at ceiling = 1 the comparison still covers every frame the reference does not set aside."""
    import evaluation as ev
    r = ev.f0_candidates_batch(batch['wav'], batch['lens'], n_cand=n_cand, ceiling=ceiling)
    y = ev.f0_batch(batch['wav'], batch['lens'])
    assert torch.equal(r.aperiodicity, y.aperiodicity) and r.frames == y.n_frames
    f0, pitch, cost, n, ap = (_np(t) for t in (r.f0, r.pitch, r.cost, r.n, r.aperiodicity))
    assert f0.shape == (len(batch['lens']), 1 + batch['wav'].shape[1] // HOP, n_cand) and n.dtype == np.int32
    slot = np.arange(n_cand)[None, None, :] >= n[:, :, None]
    assert (f0[slot] == 0).all() and (pitch[slot] == 0).all() and (cost[slot] == 1).all()
    assert (f0[~slot] > 0).all() and np.abs(pitch[~slot] - np.log2(f0[~slot].astype(np.float64))).max() <= 2.0 ** -19
    n_all = n_marg = 0
    for b, F in enumerate(r.frames):
        c64 = tr.candidates(batch['rows'][b], n_cand=n_cand, ceiling=ceiling, dp=batch['dp64'][b])
        c32 = tr.candidates(batch['rows'][b], n_cand=n_cand, ceiling=ceiling, dtype=np.float32, dp=batch['dp32'][b])
        assert (n[b, F:] == 0).all() and (ap[b, F:] == 1).all(), b
        marg = c64['marginal']
        n_all, n_marg = n_all + F, n_marg + int(marg.sum())
        if row_cap:
            assert marg.sum() <= (0.01 * F if F >= 100 else 0), (b, F, int(marg.sum()))
        used = np.arange(n_cand)[None, :] < c64['n'][:, None]
        with np.errstate(divide='ignore'):
            period = np.where(f0[b, :F] > 0, 16000.0 / np.where(f0[b, :F] > 0, f0[b, :F], 1).astype(np.float64), 0.0)
        lag_ok = np.where(used, np.abs(period - c64['lag']) <= 0.5 + 1e-4, True).all(1)
        agree = (n[b, :F] == c64['n']) & lag_ok
        assert agree[~marg].all(), (b, np.nonzero(~agree & ~marg)[0][:10])
        rest = (c32['n'] == c64['n']) & (c32['lag'] == c64['lag']).all(1)
        both = (agree & rest & ~marg)[:, None] & used
        print('row %2d  %6d frames, %d marginal, device differs on %d, restatement on %d, %d candidates compared'
              % (b, F, int(marg.sum()), int((~agree).sum()), int((~rest).sum()), int(both.sum())))
        if not both.any():
            continue
        e_c = np.abs(fr.cents(f0[b, :F][both], c64['f0'][both])).max()
        y_c = np.abs(fr.cents(c32['f0'][both], c64['f0'][both])).max()
        e_a = np.abs(cost[b, :F][both].astype(np.float64) - c64['cost'][both]).max()
        y_a = np.abs(c32['cost'][both].astype(np.float64) - c64['cost'][both]).max()
        fs, ks = np.nonzero(both)
        fl_c = max(_floor_cents(c64['dp'][f], int(c64['lag'][f, k])) for f, k in zip(fs, ks))
        fl_a = DELTA * c64['cost'][both].max()
        print('        f0 device %.3e cents, restatement %.3e (floor %.3e);  cost device %.3e, restatement %.3e (floor %.3e)'
              % (e_c, y_c, fl_c, e_a, y_a, fl_a))
        assert e_c <= 3.0 * (y_c if y_c > 0 else fl_c), (b, e_c, y_c, fl_c)
        assert e_a <= 3.0 * (y_a if y_a > 0 else fl_a), (b, e_a, y_a, fl_a)
    print('all rows: %d frames, %d marginal' % (n_all, n_marg))
    assert n_marg <= 0.01 * n_all
    z = batch['silent']                                                 # digital silence: no candidate, aperiodicity one
    assert (n[z] == 0).all() and (ap[z] == 1).all() and (f0[z] == 0).all()


# ------------------------------------------------------------------------------------------------------------- the chain
@pytest.fixture(scope='module')
def tracked(batch):
    import evaluation as ev
    return ev.f0_track_batch(batch['wav'], batch['lens']), ev.f0_candidates_batch(batch['wav'], batch['lens'])


def test_zero_transition_costs_give_yin_voicing_on_every_frame(batch):
    import evaluation as ev
    y = ev.f0_batch(batch['wav'], batch['lens'])
    for thr in (0.15, 0.4):
        t = ev.f0_track_batch(batch['wav'], batch['lens'], threshold=thr, jump_cost=0.0, switch_cost=0.0)
        yt = y if thr == 0.15 else ev.f0_batch(batch['wav'], batch['lens'], threshold=thr)
        assert torch.equal(t.f0 > 0, yt.f0 > 0) and torch.equal(t.state > 0, yt.f0 > 0), thr
        assert torch.equal(t.aperiodicity, yt.aperiodicity) and t.n_frames == yt.n_frames
        assert t.f0.dtype == yt.f0.dtype and t.f0.shape == yt.f0.shape


def test_the_device_path_is_the_float64_path_on_the_device_lattice(batch, tracked):
    """Viterbi in float64 on the lattice the device made (its float32 pitch and cost, taken as they are): the device's
    state equals it on every frame but those the reference marks marginal -- two best predecessors of a state closer
    than the float32 spacing of that frame's sums (f0_track_ref.viterbi) -- which are capped at 1 % of the batch and of
    every row of 100 frames or more, none in a shorter row.  The float32 restatement follows the device operation for
    operation: against it state and total are equal on every frame, bit for bit."""
    t, c = tracked
    state, total, f0 = _np(t.state), _np(t.total), _np(t.f0)
    pitch, cost, n, cf0 = _np(c.pitch), _np(c.cost), _np(c.n), _np(c.f0)
    n_all = n_marg = 0
    for b, F in enumerate(t.n_frames):
        s64, t64, marg = tr.viterbi(pitch[b, :F].astype(np.float64), cost[b, :F].astype(np.float64), n[b, :F], 0.15, 0.5, 0.1, details=True)
        s32, t32 = tr.viterbi(pitch[b, :F], cost[b, :F], n[b, :F], np.float32(0.15), np.float32(0.5), np.float32(0.1), np.float32)
        n_all, n_marg = n_all + F, n_marg + int(marg.sum())
        print('row %2d  %6d frames, %d marginal, device differs from float64 on %d, from the float32 restatement on %d; total %.6f / %.6f'
              % (b, F, int(marg.sum()), int((state[b, :F] != s64).sum()), int((state[b, :F] != s32).sum()), total[b], t64))
        assert marg.sum() <= (0.01 * F if F >= 100 else 0), (b, F, int(marg.sum()))
        assert np.array_equal(state[b, :F][~marg], s64[~marg]), (b, np.nonzero((state[b, :F] != s64) & ~marg)[0][:10])
        assert np.array_equal(state[b, :F], s32) and total[b] == np.float32(t32), (b, total[b], t32)
        assert (state[b, F:] == -1).all() and (f0[b, F:] == 0).all()
        assert np.array_equal(f0[b, :F], np.where(s32 > 0, cf0[b, np.arange(F), np.maximum(s32, 1) - 1], 0))
    assert n_marg <= 0.01 * n_all
    z = batch['silent']                                                 # digital silence: unvoiced throughout
    assert (f0[z] == 0).all() and (state[z, :t.n_frames[z]] == 0).all() and (n[z] == 0).all()


def test_the_weak_fundamental_is_tracked_at_its_own_octave(batch, tracked):
    """Frames more than 300 cents from the truth over f0_ref.fully_voiced_frames: the device's count is at most the
    float64 reference's plus the frames either stage's reference sets aside as marginal; f0_batch's is several times
    that (reported)."""
    import evaluation as ev
    t, c = tracked
    y = _np(ev.f0_batch(batch['wav'], batch['lens']).f0)
    f0 = _np(t.f0)
    for b, (x, f0_true, voiced) in batch['weak'].items():
        F = t.n_frames[b]
        c64 = tr.candidates(x, dp=batch['dp64'][b])
        ref, s64, _, _ = tr.track(x, cand=c64)
        marg = int(c64['marginal'].sum()) + int(tr.viterbi(c64['pitch'], c64['cost'], c64['n'], 0.15, 0.5, 0.1, details=True)[2].sum())
        g_dev, scored = tr.gross_errors(f0[b, :F], f0_true, voiced)
        g_ref, _ = tr.gross_errors(ref, f0_true, voiced)
        g_yin, _ = tr.gross_errors(y[b, :F], f0_true, voiced)
        print('row %d: %d frames scored; gross errors: f0_batch %d, f0_track_batch %d, float64 reference %d (+ %d marginal)'
              % (b, scored, g_yin, g_dev, g_ref, marg))
        assert g_dev <= g_ref + marg and 4 * g_ref <= g_yin


# ----------------------------------------------------------------------------------------------------------- bit identity
def _equal(a, b, F=None):
    return all(torch.equal(getattr(a, k) if F is None else getattr(a, k)[..., :F], getattr(b, k) if F is None else getattr(b, k)[..., :F])
               for k in ('f0', 'aperiodicity', 'state'))


def test_bit_identical_alone_twice_and_reversed(batch, tracked):
    import evaluation as ev
    t, c = tracked
    again = ev.f0_track_batch(batch['wav'], batch['lens'])
    assert _equal(t, again) and torch.equal(t.total, again.total)
    c2 = ev.f0_candidates_batch(batch['wav'], batch['lens'])
    assert all(torch.equal(getattr(c, k), getattr(c2, k)) for k in ('f0', 'pitch', 'cost', 'n', 'aperiodicity'))
    for b in (0, 4, 6, 8, 12):
        m = batch['lens'][b]
        one = ev.f0_track_batch(batch['wav'][b:b + 1, :m].contiguous(), [m])
        F = one.n_frames[0]
        assert torch.equal(one.f0[0], t.f0[b, :F]) and torch.equal(one.state[0], t.state[b, :F]) and torch.equal(one.total[0], t.total[b]), b
        oc = ev.f0_candidates_batch(batch['wav'][b:b + 1, :m].contiguous(), [m])
        assert torch.equal(oc.cost[0], c.cost[b, :F]) and torch.equal(oc.pitch[0], c.pitch[b, :F]) and torch.equal(oc.n[0], c.n[b, :F]), b
    # other strides, other tile boundaries: the short rows reversed in a narrower batch
    idx = [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13]
    sub = ev.f0_track_batch(torch.flip(batch['wav'][idx, :32000], dims=[0]).contiguous(), [batch['lens'][i] for i in idx][::-1])
    assert torch.equal(torch.flip(sub.f0, dims=[0]), t.f0[idx, :401]) and torch.equal(torch.flip(sub.state, dims=[0]), t.state[idx, :401])
    assert torch.equal(torch.flip(sub.total, dims=[0]), t.total[idx])


def test_graph_replay_with_new_contents_and_lengths(batch):
    """Both launches captured on static buffers with the lengths in device tensors, replayed after other waveforms and
    other lengths were copied into the same buffers: equal to the eager public call.  The first call is made outside the
    capture."""
    import evaluation as ev
    args = ev._f0_args(16000, HOP, W, 60.0, 400.0, 0.15, 'test')
    wav = batch['wav'][0:3, :32000].clone()
    d_len = torch.tensor([32000, 32000, 32000], dtype=torch.int32, device='cuda')
    d_fr = d_len // HOP + 1

    def launches():
        return ev._f0_track_launch(wav, d_len, d_fr, args, 8, 1.0, (0.15, 0.5, 0.1))

    launches()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = launches()

    def check(lens):
        g.replay()
        torch.cuda.synchronize()
        e = ev.f0_track_batch(wav, lens)
        assert torch.equal(out[0], e.f0) and torch.equal(out[1], e.aperiodicity) and torch.equal(out[2], e.state) and torch.equal(out[3], e.total)

    check([32000] * 3)
    wav.copy_(torch.stack([batch['wav'][12, :32000], batch['wav'][9, 16000:48000], batch['wav'][2, :32000] * 0.75]))
    new = [20000, 1, 31999]
    d_len.copy_(torch.tensor(new, dtype=torch.int32))
    d_fr.copy_(d_len // HOP + 1)
    check(new)


def test_no_host_synchronisation_inside_the_calls(batch):
    import evaluation as ev
    wav, lens = batch['wav'][:4, :32000].contiguous(), [32000, 20000, 801, 32000]
    c = ev.f0_candidates_batch(wav, lens)
    w48 = torch.repeat_interleave(wav, 3, dim=1)
    calls = (lambda: ev.f0_candidates_batch(wav, lens),
             lambda: ev.f0_viterbi_batch(c.pitch, c.cost, c.n, c.frames, f0=c.f0),
             lambda: ev.f0_track_batch(wav, lens),
             lambda: ev.score_wav_batch(wav, lens, w48, [3 * m for m in lens], CFG, wav_sr_b=48000, band=100, f0_method='viterbi'))
    for call in calls:
        call()
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        outs = [call() for call in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(outs[2].f0).all() and torch.equal(outs[1].state, outs[2].state) and torch.equal(outs[1].f0, outs[2].f0)


# -------------------------------------------------------------------------------------------------------- score_wav_batch
def test_score_wav_batch_with_the_viterbi_tracks(batch):
    """f0_method='viterbi' changes the tracks and nothing else: mcd, total, path_len and path are f0_method='yin''s bit for
    bit, the tracks are f0_track_batch's, and the seven figures are f0_metrics_batch's on those tracks along that path.
    With a voiced mask the tracks (and through the mask the path) are the Viterbi ones."""
    import evaluation as ev
    a, b = batch['weak'][12][0], batch['weak'][13][0]
    g = batch['rows'][0]
    wa, la = _pad([a, g, b[:24000]]), [len(a), len(g), 24000]
    wb, lb = _pad([b, a, g[:30000]]), [len(b), len(a), 30000]
    v = ev.score_wav_batch(wa, la, wb, lb, CFG, f0_method='viterbi')
    y = ev.score_wav_batch(wa, la, wb, lb, CFG)
    for k in ('mcd', 'total', 'path_len', 'path'):
        assert torch.equal(getattr(v, k), getattr(y, k)), k
    ta, tb = ev.f0_track_batch(wa, la), ev.f0_track_batch(wb, lb)
    assert torch.equal(v.f0_a, ta.f0) and torch.equal(v.f0_b, tb.f0)
    assert torch.equal(y.f0_a, ev.f0_batch(wa, la).f0) and not torch.equal(v.f0_a, y.f0_a)
    want = ev.f0_metrics_batch(ta.f0, tb.f0, ta.n_frames, tb.n_frames, v.path, v.path_len)
    for k in FIELDS:
        assert _same(getattr(v, k), getattr(want, k)), k
    print('weak pair: f0_rmse_cents yin %.1f, viterbi %.1f' % (float(y.f0_rmse_cents[0]), float(v.f0_rmse_cents[0])))
    f = ev.score_wav_batch(wa, la, wb, lb, CFG, align='frame', f0_method='viterbi', jump_cost=0.25, switch_cost=0.2, n_cand=4)
    t4 = ev.f0_track_batch(wa, la, jump_cost=0.25, switch_cost=0.2, n_cand=4)
    assert torch.equal(f.f0_a, t4.f0) and torch.equal(f.mcd, ev.score_wav_batch(wa, la, wb, lb, CFG, align='frame').mcd)
    m = ev.score_wav_batch(wa, la, wb, lb, CFG, mask='energy+voiced', f0_method='viterbi')
    assert torch.equal(m.f0_a, ta.f0) and torch.equal(m.f0_b, tb.f0)
