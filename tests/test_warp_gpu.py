"""Duration conversion on the device (csrc/vc_warp.hip): vc_duration_map and vc_time_warp bit for bit against the numpy
restatement of tests/warp_ref.py, one check of the warp that does not go through the restatement, graph replay, and
conversion.convert_duration_batch on the decoder that the convert_batch tests build."""
import numpy as np
import pytest
import torch

import warp_ref as wr
from test_convert_batch_gpu import N_ITER, _ragged, f32_models      # noqa: F401  (f32_models: a module-scoped fixture)
from test_warp_cpu import random_table

pytestmark = pytest.mark.gpu

Q = wr.Q
POISON = 0x7FC00000                     # a NaN's bits: what an unwritten int32 output would still hold
N_LIST = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)
NSEG_LIST = (0, 1, 2, 255, 256, 257, 1024, 1025)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run_map(lens, start, end, n_seg, labels=None, out_len=None, ratio_q=None, gap_q=Q, min_frames=1, Fw=None, in_frames=None):
    """vc_duration_map itself on outputs that hold NaN bits; returns warp_ref.Map of numpy arrays and checks that the
    inputs are what they were."""
    import _vc
    lib = _vc.lib()
    B, K = start.shape
    ins = [np.asarray(a, np.int32) if a is not None else None for a in (start, end, n_seg, labels, out_len, ratio_q, lens)]
    d = [None if a is None else _dev(a) for a in ins]
    pos = torch.full((B, Fw), POISON, dtype=torch.int32, device='cuda')
    tab = torch.full((2, B, K), POISON, dtype=torch.int32, device='cuda')
    small = torch.full((2, B), POISON, dtype=torch.int32, device='cuda')
    need = lib.vc_duration_map_workspace_bytes(B, K)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device='cuda')
    _vc.check(lib.vc_duration_map(_vc.ptr(d[0]), _vc.ptr(d[1]), _vc.ptr(d[2]), _vc.ptr(d[3]), _vc.ptr(d[4]), _vc.ptr(d[5]),
                                  0 if ratio_q is None else len(ratio_q), int(gap_q), _vc.ptr(d[6]), B, K,
                                  int(in_frames or max(int(np.max(lens)), 1)), int(min_frames), Fw, _vc.ptr(pos), _vc.ptr(small[0]),
                                  _vc.ptr(tab[0]), _vc.ptr(tab[1]), _vc.ptr(small[1]), _vc.ptr(ws), need, _vc.current_stream()))
    torch.cuda.synchronize()
    for a, t in zip(ins, d):
        assert a is None or np.array_equal(t.cpu().numpy(), a)
    return wr.Map(pos.cpu().numpy(), small[0].cpu().numpy(), tab[0].cpu().numpy(), tab[1].cpu().numpy(), small[1].cpu().numpy())


def same_map(got, want, what=''):
    for name, g, w in zip(wr.Map._fields, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError('%s %s: %d of %d differ, first at %s: device %s, reference %s'
                                 % (what, name, len(bad), g.size, bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def seam_table(rng, n, n_seg, K):
    """n_seg table entries for an utterance of n frames: as many present segments as fit, placed at random entries, the
    others absent (-1 or empty); gaps at either end or not; entries from n_seg on hold junk."""
    s, e, m = random_table(rng, n, min(n_seg, max(n, 1)), p_absent=0.0)
    start, end = np.full(K, 12345, np.int32), np.full(K, -777, np.int32)
    start[:n_seg], end[:n_seg] = -1, -1
    empty = rng.rand(n_seg) < 0.5
    v = rng.randint(0, n + 1, n_seg)
    start[:n_seg][empty], end[:n_seg][empty] = v[empty], v[empty]
    at = np.sort(rng.choice(n_seg, size=m, replace=False)) if m else np.zeros(0, np.int64)
    start[at], end[at] = s[:m], e[:m]
    return start, end


@pytest.fixture(scope='module')
def seam_batch():
    """Every n x n_seg of the seams (lanes per workgroup, tile of 1,024 entries) as one ragged batch."""
    rng = np.random.RandomState(7)
    K = 1030
    lens, n_seg, start, end = [], [], [], []
    for n in N_LIST:
        for ns in NSEG_LIST:
            s, e = seam_table(rng, n, ns, K)
            lens.append(n); n_seg.append(ns); start.append(s); end.append(e)
    C = 9
    return dict(lens=np.array(lens, np.int32), n_seg=np.array(n_seg, np.int32), start=np.stack(start), end=np.stack(end), K=K, C=C,
                labels=rng.randint(0, C, (len(lens), K)).astype(np.int32),
                out_len=rng.choice([0, 0, 1, 2, 3, 7], (len(lens), K)).astype(np.int32),
                ratio_q=wr.ratio_to_q([0.0, 0.5, 1.0, 1.3, 2.0, 8.0, 0.77, 1.0, 3.01]))


@pytest.mark.parametrize('how', ['labels', 'one_rate', 'out_len', 'plain'])
def test_duration_map_bit_exact_at_the_seams(seam_batch, how):
    b = seam_batch
    kw = dict(labels=dict(labels=b['labels'], ratio_q=b['ratio_q'], gap_q=int(1.5 * Q)), one_rate=dict(ratio_q=[int(1.3 * Q)], gap_q=Q // 2),
              out_len=dict(out_len=b['out_len'], gap_q=Q), plain=dict(gap_q=2 * Q))[how]
    Fw = 1500                                                       # some utterances exceed it (flag 4), most do not
    got = run_map(b['lens'], b['start'], b['end'], b['n_seg'], Fw=Fw, min_frames=2, **kw)
    want = wr.duration_map_batch(b['lens'], b['start'], b['end'], b['n_seg'], Fw_max=Fw, min_frames=2, **kw)
    same_map(got, want, how)
    assert not (want.flags & wr.FLAG_INVALID).any() and (want.flags & wr.FLAG_SHORT).any()
    assert how != 'labels' or (want.flags & wr.FLAG_TRUNCATED).any()
    if how == 'labels':                                             # each utterance alone, under another K, Fw and batch
        for i in (3, 11, 40, 47, 63, 87):
            n, ns = int(b['lens'][i]), int(b['n_seg'][i])
            K1 = max(ns, 1)
            one = run_map(b['lens'][i:i + 1], b['start'][i:i + 1, :K1], b['end'][i:i + 1, :K1], b['n_seg'][i:i + 1], Fw=Fw + 5,
                          min_frames=2, labels=b['labels'][i:i + 1, :K1], ratio_q=b['ratio_q'], gap_q=int(1.5 * Q))
            if not want.flags[i] & wr.FLAG_TRUNCATED:
                assert np.array_equal(one.pos[0, :Fw], got.pos[i]) and one.n_out[0] == got.n_out[i] and one.flags[0] == got.flags[i]
                assert np.array_equal(one.out_start[0], got.out_start[i, :K1]) and np.array_equal(one.out_end[0], got.out_end[i, :K1])


def test_duration_map_invalid_tables_flags_and_limits():
    n = 40
    rows = [([0, 10, 20], [10, 20, 30]),                            # valid, for comparison
            ([10, 0, 20], [20, 10, 30]),                            # unsorted
            ([0, 9, 20], [10, 20, 30]),                             # overlapping
            ([0, 10, 20], [10, 20, 41]),                            # outside [0, n]
            ([0, 15, 20], [10, 12, 30]),                            # end < start
            ([0, 10, 2 ** 31 - 1], [10, 20, -2 ** 31]),             # wild values: nothing may be indexed with them
            ([-5, 10, 20], [3, 20, 30]),                            # start < 0: absent, not invalid
            ([0, 10, 20], [10, 10, 30])]                            # an empty segment: absent
    start, end = (np.array([r[i] for r in rows], np.int32) for i in (0, 1))
    B = len(rows)
    lens, n_seg = np.full(B, n, np.int32), np.full(B, 3, np.int32)
    rq = [int(1.5 * Q)]
    got = run_map(lens, start, end, n_seg, ratio_q=rq, Fw=100)
    want = wr.duration_map_batch(lens, start, end, n_seg, ratio_q=rq, Fw_max=100)
    same_map(got, want)
    assert want.flags.tolist() == [0, 1, 1, 1, 1, 1, 0, 0]
    for b in range(1, 6):
        assert got.n_out[b] == n and np.array_equal(got.pos[b, :n], np.arange(n) * Q) and (got.out_start[b] == -1).all()
    # labels outside the rate table and negative explicit lengths
    labels = np.array([[0, 1, 2], [0, 3, 1], [-1, 0, 0], [2 ** 30, 0, 0]], np.int32)
    s4, e4 = np.tile(start[:1], (4, 1)), np.tile(end[:1], (4, 1))
    rq3 = wr.ratio_to_q([1.0, 2.0, 0.5])
    got = run_map(lens[:4], s4, e4, n_seg[:4], labels=labels, ratio_q=rq3, Fw=100)
    same_map(got, wr.duration_map_batch(lens[:4], s4, e4, n_seg[:4], labels=labels, ratio_q=rq3, Fw_max=100))
    assert got.flags.tolist() == [0, 1, 1, 1]
    ol = np.array([[3, 0, 5], [3, -1, 5], [0, 0, 0], [2 ** 31 - 1, 2 ** 31 - 1, 7]], np.int32)      # deletions; a sum beyond 32 bits
    got = run_map(lens[:4], s4, e4, n_seg[:4], out_len=ol, Fw=100, gap_q=0)
    same_map(got, wr.duration_map_batch(lens[:4], s4, e4, n_seg[:4], out_len=ol, Fw_max=100, gap_q=0))
    assert got.flags.tolist() == [0, 1, 2, 4] and got.n_out.tolist() == [8, n, n, 100]
    # rates in the table beyond [0, 8] are clamped when read
    wild = np.array([-5, 2 ** 31 - 1, 9 * Q], np.int32)
    got = run_map(lens[:1], s4[:1], e4[:1], n_seg[:1], labels=labels[:1], ratio_q=wild, Fw=400)
    same_map(got, wr.duration_map_batch(lens[:1], s4[:1], e4[:1], n_seg[:1], labels=labels[:1], ratio_q=wild, Fw_max=400))
    assert got.n_out[0] == 0 + 80 + 80 + 10
    # totals at min_frames and at Fw: 40 frames at 1.5 -> 60
    for mf, Fw, fl, n_out in ((60, 60, 0, 60), (61, 61, wr.FLAG_SHORT, 40), (1, 59, wr.FLAG_TRUNCATED, 59), (61, 39, 6, 39)):
        got = run_map(lens[:1], start[:1], end[:1], n_seg[:1], ratio_q=rq, gap_q=rq[0], min_frames=mf, Fw=Fw)
        same_map(got, wr.duration_map_batch(lens[:1], start[:1], end[:1], n_seg[:1], ratio_q=rq, gap_q=rq[0], min_frames=mf, Fw_max=Fw))
        assert (int(got.flags[0]), int(got.n_out[0])) == (fl, n_out)
    # counts beyond the arrays are clamped: n_seg to K, n to the launch's max_frames
    got = run_map(np.array([10 ** 6], np.int32), start[:1], end[:1], np.array([99], np.int32), ratio_q=rq, Fw=100, in_frames=40)
    same_map(got, wr.duration_map_batch(lens[:1], start[:1], end[:1], n_seg[:1], ratio_q=rq, Fw_max=100))


def test_duration_map_at_the_limits():
    """16,384 single-frame segments in 16,384 frames, each rounding 1.5 up to 2: the offsets pass the output bound after
    half the table; and one segment over everything stretched eightfold."""
    n = 16384
    k = np.arange(n, dtype=np.int32)
    start, end = np.stack([k, np.zeros(n, np.int32)]), np.stack([k + 1, np.r_[n, np.zeros(n - 1)].astype(np.int32)])
    lens, n_seg = np.array([n, n], np.int32), np.array([n, 1], np.int32)
    labels = np.zeros((2, n), np.int32)
    labels[1, 0] = 1
    rq = [3 * Q // 2, 8 * Q]
    got = run_map(lens, start, end, n_seg, labels=labels, ratio_q=rq, Fw=n)
    want = wr.duration_map_batch(lens, start, end, n_seg, labels=labels, ratio_q=rq, Fw_max=n)
    same_map(got, want)
    assert got.flags.tolist() == [4, 4] and got.n_out.tolist() == [n, n] and got.pos[0, -1] >> 16 == n // 2 - 1 and got.pos[1, -1] >> 16 == n // 8 - 1


# ----------------------------------------------------------------------------------------------------- the warp
def run_warp(x, pos, n_out, lens, mode, norm=None):
    import _vc
    B, F, C = x.shape
    Fw = pos.shape[1]
    d_x, d_pos, d_no, d_len = _dev(x), _dev(pos.astype(np.int32)), _dev(np.asarray(n_out, np.int32)), _dev(np.asarray(lens, np.int32))
    out = torch.full((B, Fw, C), float('nan'), device='cuda')
    amp = torch.full((B, Fw, C), float('nan'), device='cuda') if norm else None
    _vc.check(_vc.lib().vc_time_warp(_vc.ptr(d_x), _vc.ptr(d_pos), _vc.ptr(d_no), _vc.ptr(d_len), B, F, Fw, C, mode, _vc.ptr(out),
                                     _vc.ptr(amp), float(norm or 0.0), _vc.current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy(), x, equal_nan=True) and np.array_equal(d_pos.cpu().numpy(), pos)
    return out, amp, d_no


def warp_case(rng, F, Fw):
    """Four utterances: stretched and squeezed by a table, the identity, an empty one, and every second frame; pos beyond
    n_out holds junk."""
    lens = np.array([F, F - 7, 0, F], np.int32)
    pos = rng.randint(-2 ** 31, 2 ** 31 - 1, (4, Fw), dtype=np.int64).astype(np.int32)
    m = wr.duration_map(F, np.array([5, 30]), np.array([22, F - 3]), 2, labels=np.array([0, 1]), ratio_q=wr.ratio_to_q([2.3, 0.61]),
                        gap_q=Q, Fw_max=Fw)
    n_out = np.array([m.n_out, F - 7, 13, F // 2], np.int32)
    pos[0, :m.n_out] = m.pos[:m.n_out]
    pos[1, :F - 7] = np.arange(F - 7) * Q
    pos[3, :F // 2] = 2 * np.arange(F // 2) * Q
    return lens, pos, n_out


@pytest.mark.parametrize('C', [1, 3, 4, 61, 80, 201, 204])
def test_time_warp_bit_exact(C):
    import _vc
    rng = np.random.RandomState(C)
    F = 70
    for Fw in (96, 97):                                             # 16-byte stores on the flat slab; a slab of odd length
        lens, pos, n_out = warp_case(rng, F, Fw)
        x = rng.uniform(-0.2, 0.9, (4, F, C)).astype(np.float32)
        x[1, F - 7:] = np.nan                                       # never read beyond the utterance's own frames ...
        x[3, 1::2] = np.nan                                         # ... nor the neighbour row where the weight is 0
        for mode, name in ((0, 'linear'), (1, 'nearest')):
            out, amp, d_no = run_warp(x, pos, n_out, lens, mode, norm=0.01)
            got = out.cpu().numpy()
            for b in range(4):
                want = wr.time_warp(x[b], pos[b], n_out[b], lens[b], name)
                assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (C, Fw, name, b)
                assert not got[b, n_out[b] if lens[b] else 0:].any()
            assert np.array_equal(got[1, :F - 7], x[1, :F - 7])     # the identity map returns the source
            assert np.array_equal(got[3, :F // 2], x[3, ::2]) and np.isfinite(got).all()
            # the fused magnitude is vc_power_to_amp of the warped spectrum
            want_amp = torch.full_like(out, float('nan'))
            n_eff = torch.where(_dev(lens) > 0, d_no, torch.zeros_like(d_no))
            _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(out), _vc.ptr(n_eff), 4, Fw, C, 0.01, 1.0, _vc.ptr(want_amp), _vc.current_stream()))
            assert torch.equal(amp, want_amp) and float(amp[1].max()) > 1e-4
            plain, none, _ = run_warp(x, pos, n_out, lens, mode)
            assert none is None and torch.equal(plain, out)


@pytest.mark.parametrize('C', [4, 201])
def test_time_warp_of_a_ramp_is_the_map_itself(C):
    """Independent of the restatement: a source whose row f holds f * 2^-4 warped linearly must hold pos * 2^-20 exactly
    (both exact in float32: 14 integer bits of frame, 16 of fraction would not be, so the ramp stays below 256 frames)."""
    import conversion
    F = 250
    rng = np.random.RandomState(1)
    start, end, n_seg = random_table(rng, F, 40)
    labels = rng.randint(0, 5, (1, 40)).astype(np.int32)
    m = conversion.duration_map_batch(start[None], end[None], [n_seg], [F], labels=labels, ratio=[0.5, 1.0, 1.37, 2.0, 3.3], gap_ratio=0.8)
    x = np.repeat((np.arange(F, dtype=np.float32) * np.float32(2.0 ** -4))[None, :, None], C, 2)
    y = conversion.time_warp_batch(x, m.pos, m.n_out, [F])
    n_out = int(m.n_out[0])
    assert int(m.flags[0]) == 0 and n_out > F // 2 and y.shape == (1, m.max_frames, C)
    want = m.pos[0, :n_out].to(torch.float32) * 2.0 ** -20
    assert torch.equal(y[0, :n_out], want[:, None].expand(n_out, C)) and not y[0, n_out:].any()
    assert len(torch.unique(m.pos[0, :n_out] & 65535)) > 20        # fractional positions took part


def test_duration_map_batch_wrapper_and_device_ratio():
    """The Python entry point on host arrays and on device tensors gives the restatement's map; a float ratio on the
    device is rounded to Q16 there as the host rounds it."""
    import conversion
    rng = np.random.RandomState(2)
    B, K, F = 4, 30, 180
    tabs = [random_table(rng, F - 10 * b, K) for b in range(B)]
    start, end, n_seg = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), np.array([t[2] for t in tabs], np.int32)
    lens = np.array([F - 10 * b for b in range(B)], np.int32)
    labels = rng.randint(0, 6, (B, K)).astype(np.int32)
    ratio = np.array([0.3, 0.999999, 1.0000001, 1.5, 2.71828, 8.0], np.float32)
    a = conversion.duration_map_batch(start, end, n_seg, lens, labels=labels, ratio=ratio, gap_ratio=1.25, min_frames=4)
    Fw = conversion.duration_max_frames(F, 2 * K + 1, 8 * Q)
    assert a.max_frames == Fw
    want = wr.duration_map_batch(lens, start, end, n_seg, labels=labels, ratio_q=wr.ratio_to_q(ratio), gap_q=int(1.25 * Q), min_frames=4, Fw_max=Fw)
    same_map(wr.Map(*(t.cpu().numpy() for t in a[:5])), want)
    b = conversion.duration_map_batch(_dev(start), _dev(end), _dev(n_seg), _dev(lens), labels=_dev(labels), ratio=_dev(ratio),
                                      gap_ratio=1.25, min_frames=4, max_frames=Fw)
    same_map(wr.Map(*(t.cpu().numpy() for t in b[:5])), want)
    with pytest.raises(ValueError, match='max_frames'):
        conversion.duration_map_batch(_dev(start), _dev(end), _dev(n_seg), _dev(lens))
    st = conversion.duration_stats_batch(_dev(labels), _dev(start), _dev(end), _dev(n_seg), 6)
    cnt, tot = np.zeros(6, np.int64), np.zeros(6, np.int64)
    for i in range(B):
        for k in range(n_seg[i]):
            if start[i, k] >= 0 and end[i, k] > start[i, k]:
                cnt[labels[i, k]] += 1
                tot[labels[i, k]] += end[i, k] - start[i, k]
    assert st.count.is_cuda and st.count.tolist() == cnt.tolist() and st.total.tolist() == tot.tolist()


def test_graph_replay_of_map_and_warp():
    import conversion
    from test_graph_replay_gpu import _capture, _free, _same
    rng = np.random.RandomState(3)
    B, K, F, C, Fw = 3, 40, 300, 201, 700

    def inputs(k):
        lens = np.array([F, F - 31 * (k + 1), 17 + k], np.int32)
        tabs = [random_table(rng, int(n), K) for n in lens]
        return [_dev(np.stack([t[0] for t in tabs])), _dev(np.stack([t[1] for t in tabs])), _dev(np.array([t[2] for t in tabs], np.int32)),
                _dev(lens), _dev(rng.randint(0, 4, (B, K)).astype(np.int32)), _dev(rng.uniform(0.3, 2.5, 4).astype(np.float32)),
                _dev(rng.uniform(-0.2, 0.9, (B, F, C)).astype(np.float32))]

    def chain(start, end, n_seg, lens, labels, ratio, x):
        m = conversion.duration_map_batch(start, end, n_seg, lens, labels=labels, ratio=ratio, max_frames=Fw, min_frames=4)
        y, amp = conversion.time_warp_batch(x, m.pos, m.n_out, lens, P_dB_norm_factor=0.01)
        return m.pos, m.n_out, m.out_start, m.out_end, m.flags, y, amp

    static = inputs(0)
    g, outs = _capture(lambda: chain(*static))
    try:
        for k in range(1, 4):
            new = inputs(k)
            for s, t in zip(static, new):
                s.copy_(t)
            g.replay()
            torch.cuda.synchronize()
            want = chain(*new)
            for name, a, b in zip(('pos', 'n_out', 'out_start', 'out_end', 'flags', 'warped', 'amp'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert int(outs[1][0]) > 0 and float(outs[6][0, 0].max()) > 0
    finally:
        _free(g)


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def plain_run(f32_models):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_batch(dec, wav, lens, c, n_iter=N_ITER, phase='device', seed=5)
    torch.cuda.synchronize()
    return r


def test_rate_one_is_convert_batch(f32_models, plain_run):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_duration_batch(dec, wav, lens, c, rate=1.0, n_iter=N_ITER, phase='device', seed=5)
    assert r.max_frames == 1200 and r.max_samples == 80 * 1199 and r.src_frames == plain_run.n_frames
    assert r.n_frames.tolist() == plain_run.n_frames and r.n_samples.tolist() == plain_run.n_samples and r.flags.tolist() == [0, 0, 0]
    for name in ('mel_pred', 'stft_pred', 'phn_pred', 'y_wav_pred'):
        assert torch.equal(getattr(r, name), getattr(plain_run, name)), name
    assert r.seg.start.tolist() == [[0]] * 3 and r.seg.end[:, 0].tolist() == plain_run.n_frames


@pytest.mark.parametrize('rate', [0.5, 2.0])
def test_rate_changes_the_length(f32_models, plain_run, rate):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_duration_batch(dec, wav, lens, c, rate=rate, n_iter=N_ITER, seed=5)
    want = [wr.duration_map(n, [0], [n], 1, ratio_q=wr.ratio_to_q([rate]), min_frames=4, Fw_max=2 * n) for n in plain_run.n_frames]
    n_out = [m.n_out for m in want]
    assert n_out == [int(n * rate) for n in plain_run.n_frames] and r.max_frames == max(n_out)
    assert r.n_frames.tolist() == n_out and r.n_samples.tolist() == [80 * (n - 1) for n in n_out] and r.flags.tolist() == [0, 0, 0]
    assert r.y_wav_pred.shape == (3, 80 * (max(n_out) - 1)) and torch.isfinite(r.y_wav_pred).all()
    for b, m in enumerate(want):
        assert np.array_equal(r.map.pos[b, :m.n_out].cpu().numpy(), m.pos[:m.n_out]) and not r.y_wav_pred[b, 80 * (m.n_out - 1):].any()
        assert float(r.y_wav_pred[b, :80 * (m.n_out - 1)].abs().mean()) == pytest.approx(0.045, abs=1e-4)
        w = wr.time_warp(plain_run.stft_pred[b].cpu().numpy(), m.pos, m.n_out, plain_run.n_frames[b])
        assert np.array_equal(r.stft_pred[b, :m.n_out].cpu().numpy(), w[:m.n_out]) and not r.stft_pred[b, m.n_out:].any()


def test_decoded_segments_with_a_rate_table_equal_the_separate_calls(f32_models, plain_run):
    import conversion
    import evaluation
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    ratio = np.random.RandomState(9).choice([0.5, 0.8, 1.25, 2.0], 61).astype(np.float32)
    r = conversion.convert_duration_batch(dec, wav, lens, c, ratio=ratio, gap_ratio=0.75, n_iter=N_ITER, seed=5, decode=dict(min_dur=2))
    d = evaluation.decode_batch(plain_run.phn_pred, plain_run.n_frames, min_dur=2)
    m = conversion.duration_map_batch(d.seg.start, d.seg.end, d.seg.n_seg, plain_run.n_frames, labels=d.seg.labels, ratio=ratio,
                                      gap_ratio=0.75, max_frames=r.max_frames, min_frames=conversion.duration_min_frames(c))
    assert r.max_frames == conversion.duration_max_frames(1200, 2401, int(wr.ratio_to_q(ratio).max())) and int(d.seg.n_seg.min()) >= 1
    assert torch.equal(r.n_frames, m.n_out) and torch.equal(r.map.pos, m.pos) and r.flags.tolist() == [0, 0, 0]
    assert torch.equal(r.seg.start, m.out_start) and torch.equal(r.seg.end, m.out_end) and torch.equal(r.seg.labels, d.seg.labels)
    assert r.n_frames.tolist() != plain_run.n_frames
    for name in ('mel_pred', 'stft_pred', 'phn_pred'):
        want = conversion.time_warp_batch(getattr(plain_run, name), m.pos, m.n_out, plain_run.n_frames)
        assert torch.equal(getattr(r, name), want), name
    n_out = r.n_frames.tolist()
    assert torch.isfinite(r.y_wav_pred).all() and all(not r.y_wav_pred[b, 80 * (n_out[b] - 1):].any() for b in range(3))
    # a given table (here the decoded one) and explicit lengths: every segment two frames longer
    tab = (d.seg.labels, d.seg.start, d.seg.end, d.seg.n_seg)
    ol = torch.where(d.seg.start >= 0, d.seg.end - d.seg.start + 2, torch.zeros_like(d.seg.start))
    r2 = conversion.convert_duration_batch(dec, wav, lens, c, out_len=ol, segments=tab, max_frames=3000, n_iter=N_ITER, seed=5, realse=1.2)
    assert r2.n_frames.tolist() == [n + 2 * int(k) for n, k in zip(plain_run.n_frames, d.seg.n_seg.tolist())]
    assert torch.isfinite(r2.y_wav_pred).all() and r2.stft_pred.shape == (3, 3000, 201)


def test_no_host_synchronisation_and_argument_checks(f32_models, plain_run):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    d_wav = _dev(wav)
    ratio = _dev(np.linspace(0.6, 1.4, 61).astype(np.float32))
    calls = (dict(rate=1.5), dict(ratio=ratio, max_frames=2400, gap_ratio=1.2), dict(rate=0.75, phase='spsi', out_sr=22050))
    for kw in calls:                                                # warm-up
        conversion.convert_duration_batch(dec, d_wav, lens, c, n_iter=N_ITER, window_batch=4, **kw)
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()
        rs = [conversion.convert_duration_batch(dec, d_wav, lens, c, n_iter=N_ITER, window_batch=4, **kw) for kw in calls]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.y_wav_pred).all() for r in rs) and rs[1].flags.tolist() == [0, 0, 0]
    n2 = rs[2].n_frames.tolist()
    assert rs[2].n_samples.tolist() == [-(-80 * (n - 1) * 441 // 320) for n in n2] and rs[2].max_samples == -(-80 * (max(n2) - 1) * 441 // 320)
    for kw, msg in ((dict(rate=1.0, phase='numpy'), 'phase'), (dict(rate=0.0), 'rate'), (dict(rate=8.5), 'rate'), (dict(rate=float('nan')), 'rate'),
                    (dict(rate=True), 'rate'), (dict(ratio=[1.0] * 61, out_len=np.zeros((3, 1200), np.int32)), 'exactly one'),
                    (dict(rate=1.0, ratio=[1.0] * 61), 'exactly one'), (dict(), 'exactly one'), (dict(rate=0.005), 'vocoder'),
                    (dict(ratio=ratio), 'max_frames'), (dict(rate=1.0, mode='cubic'), 'mode'), (dict(rate=1.0, decode=dict(min_dur=2)), 'decode'),
                    (dict(ratio=[1.0] * 61, segments='argmax'), 'segments')):
        with pytest.raises(ValueError, match=msg):
            conversion.convert_duration_batch(dec, d_wav, lens, c, n_iter=N_ITER, **kw)
