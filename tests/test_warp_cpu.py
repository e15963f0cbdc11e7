"""The duration map's definition (tests/warp_ref.py) against what it stands for, without a GPU: the centre-aligned map
in float64, monotony, the identity, the rounding rule of the output table, every flag bit, the default output bound, and
the host-side helpers of conversion.py."""
import numpy as np
import pytest
import torch

import warp_ref as wr

Q = wr.Q


def random_table(rng, n, K, p_absent=0.2, touch=0.3):
    """A valid table of up to K entries inside [0, n]: sorted, disjoint, some entries absent (-1 or empty), some segments
    touching, gaps at either end or not."""
    cuts = np.sort(rng.choice(np.arange(n + 1), size=min(2 * K, n + 1), replace=False)) if n > 0 else np.zeros(0, np.int64)
    start, end = np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    k = i = 0
    while k < K and i + 1 < len(cuts):
        r = rng.rand()
        if r < p_absent / 2:
            k += 1                                                  # skipped optional state: -1, -1
            continue
        if r < p_absent:
            start[k] = end[k] = cuts[i]                             # an empty segment
            k += 1
            continue
        start[k], end[k] = cuts[i], cuts[i + 1]
        i += 1 if rng.rand() < touch else 2                         # the next one starts where this ends, or after a gap
        k += 1
    return start, end, k


def test_map_is_the_centre_aligned_map_monotone_and_inside():
    rng = np.random.RandomState(0)
    for it in range(300):
        n = int(rng.randint(1, 400))
        K = int(rng.randint(1, 40))
        start, end, n_seg = random_table(rng, n, K)
        C = 7
        labels = rng.randint(0, C, K).astype(np.int32)
        ratio_q = wr.ratio_to_q(rng.choice([0.0, 0.5, 1.0, 1.3, 2.0, 8.0, 0.77], C))
        gap_q = int(wr.ratio_to_q(rng.choice([0.0, 0.5, 1.0, 1.7])))
        if it % 3 == 0:
            kw = dict(out_len=rng.randint(0, 30, K).astype(np.int32), gap_q=gap_q)
        else:
            kw = dict(labels=labels, ratio_q=ratio_q, gap_q=gap_q)
        P = wr.pieces(n, start, end, n_seg, **kw)
        assert P is not None
        total = sum(p[3] for p in P)
        m = wr.duration_map(n, start, end, n_seg, min_frames=0, Fw_max=total + 3, **kw)
        assert m.flags == 0 and m.n_out == total and (m.pos[total:] == -1).all()
        pos = m.pos[:total].astype(np.int64)
        want = np.clip(wr.center_map_f64(P), 0.0, n - 1.0)
        assert np.abs(pos / Q - want).max() <= 2.0 ** -16 if total else True
        assert (np.diff(pos) >= 0).all() and (pos >= 0).all() and (pos <= (n - 1) * Q).all()
        # the output table tiles [0, n_out) together with the gaps, in order
        edge = 0
        for S, Li, O, Lo, k in P:
            assert O == edge
            edge += Lo
            if k >= 0:
                assert (m.out_start[k], m.out_end[k]) == (O, O + Lo)
        assert edge == m.n_out
        absent = [k for k in range(K) if k >= n_seg or start[k] < 0 or end[k] == start[k]]
        assert (m.out_start[absent] == -1).all() and (m.out_end[absent] == -1).all()


def test_identity_at_unit_rates():
    rng = np.random.RandomState(1)
    for _ in range(50):
        n, K = int(rng.randint(1, 300)), int(rng.randint(1, 30))
        start, end, n_seg = random_table(rng, n, K)
        m = wr.duration_map(n, start, end, n_seg, labels=np.zeros(K, np.int32), ratio_q=[Q], gap_q=Q)
        assert m.flags == 0 and m.n_out == n and np.array_equal(m.pos, np.arange(n) * Q)
        present = (start[:n_seg] >= 0) & (end[:n_seg] > start[:n_seg])
        assert np.array_equal(m.out_start[:n_seg][present], start[:n_seg][present])
        assert np.array_equal(m.out_end[:n_seg][present], end[:n_seg][present])


@pytest.mark.parametrize('ratio', [0.0, 0.5, 1.0, 1.3, 2.0, 8.0])
def test_output_lengths_follow_the_rounding_rule(ratio):
    start = np.array([2, 7, 8, 20, -1, 31], np.int32)
    end = np.array([7, 8, 19, 31, -1, 31], np.int32)                # touching, a gap, a skipped entry, an empty one
    n = 40
    rq = wr.ratio_to_q([ratio])
    assert int(rq[0]) == int(round(ratio * Q))
    m = wr.duration_map(n, start, end, 6, ratio_q=rq, gap_q=Q, min_frames=0, Fw_max=8 * n + 8)
    lens = (m.out_end - m.out_start)[:4]
    assert lens.tolist() == [(int(L) * int(rq[0]) + 32768) >> 16 for L in (5, 1, 11, 11)]
    gaps = 2 + 1 + 9                                                # [0, 2), [19, 20), [31, 40) at rate 1
    assert m.n_out == lens.sum() + gaps and m.flags == 0
    assert m.out_start[4] == m.out_end[4] == -1 and m.out_start[5] == m.out_end[5] == -1
    # the ranges tile [0, n_out) with the gaps between them
    assert m.out_start[0] == 2 and m.out_start[2] == m.out_end[1] and m.out_start[3] == m.out_end[2] + 1
    assert m.out_end[3] + 9 == m.n_out


def test_every_flag_bit():
    s, e = np.array([0, 10], np.int32), np.array([10, 20], np.int32)
    ident = np.arange(30) * Q
    for bad_s, bad_e in (([10, 0], [20, 10]), ([0, 5], [10, 20]), ([0, 10], [10, 31]), ([5, 10], [4, 20])):   # unsorted, overlap, outside, end < start
        m = wr.duration_map(30, np.array(bad_s), np.array(bad_e), 2, ratio_q=[2 * Q], Fw_max=100)
        assert m.flags == wr.FLAG_INVALID and m.n_out == 30 and np.array_equal(m.pos[:30], ident) and (m.out_start == -1).all()
    m = wr.duration_map(30, s, e, 2, labels=np.array([0, 3]), ratio_q=[Q, Q], Fw_max=100)      # a label outside the table
    assert m.flags == wr.FLAG_INVALID
    m = wr.duration_map(30, s, e, 2, out_len=np.array([3, -1]), Fw_max=100)
    assert m.flags == wr.FLAG_INVALID
    # below min_frames: 30 frames at rate 0.25 -> 3 + 3 + 3 (2.5 rounds up; the last is the gap at gap_q) = 9 < 10
    q4 = Q // 4
    m = wr.duration_map(30, s, e, 2, ratio_q=[q4], gap_q=q4, min_frames=10, Fw_max=100)
    assert m.flags == wr.FLAG_SHORT and m.n_out == 30 and np.array_equal(m.pos[:30], ident)
    assert m.out_start.tolist() == [0, 10] and m.out_end.tolist() == [10, 20]
    m = wr.duration_map(30, s, e, 2, ratio_q=[q4], gap_q=q4, min_frames=9, Fw_max=100)
    assert m.flags == 0 and m.n_out == 9
    # above Fw_max: 60 frames wanted, 59 allowed; exactly 60 allowed
    m = wr.duration_map(30, s, e, 2, ratio_q=[2 * Q], gap_q=2 * Q, Fw_max=59)
    assert m.flags == wr.FLAG_TRUNCATED and m.n_out == 59 and m.out_end.tolist() == [20, 40] and (m.pos >= 0).all()
    full = wr.duration_map(30, s, e, 2, ratio_q=[2 * Q], gap_q=2 * Q, Fw_max=60)
    assert full.flags == 0 and full.n_out == 60 and np.array_equal(full.pos[:59], m.pos)
    m = wr.duration_map(30, s, e, 2, ratio_q=[2 * Q], gap_q=2 * Q, Fw_max=35)
    assert m.flags == wr.FLAG_TRUNCATED and m.out_start.tolist() == [0, 20] and m.out_end.tolist() == [20, 35]
    # the identity map can be cut as well: both bits
    m = wr.duration_map(30, np.array([10, 0]), np.array([20, 10]), 2, Fw_max=12)
    assert m.flags == wr.FLAG_INVALID | wr.FLAG_TRUNCATED and m.n_out == 12
    m = wr.duration_map(0, s, e, 2, ratio_q=[2 * Q], Fw_max=10)
    assert m.flags == 0 and m.n_out == 0 and (m.pos == -1).all() and (m.out_start == -1).all()
    # deletions: an explicit length of 0 gives an empty range and the neighbours close up
    m = wr.duration_map(30, s, e, 2, out_len=np.array([0, 4]), Fw_max=100)
    assert m.flags == 0 and m.n_out == 14 and m.out_start.tolist() == [0, 0] and m.out_end.tolist() == [0, 4]
    assert m.pos[0] >> 16 >= 10


def test_default_bound_never_truncates():
    import conversion
    rng = np.random.RandomState(3)
    worst = 0
    for it in range(400):
        n, K = int(rng.randint(1, 200)), int(rng.randint(1, 24))
        start, end, n_seg = random_table(rng, n, K, touch=0.5)
        C = 5
        ratio = rng.choice([0.0, 0.49, 0.5, 1.0, 1.25, 1.5, 2.0, 2.5, 7.99, 8.0], C).astype(np.float32)
        if it % 4 == 0:
            ratio = np.full(C, rng.choice([1.5, 2.5, 0.5]), np.float32)      # every piece rounds up at odd lengths
        gap = float(rng.choice([0.0, 0.5, 1.0, 1.5, 2.5]))
        rq, gq = conversion.ratio_to_q(ratio), int(conversion.ratio_to_q(gap))
        assert np.array_equal(rq, wr.ratio_to_q(ratio))
        Fw = conversion.duration_max_frames(n, 2 * K + 1, max(int(rq.max()), gq))
        labels = rng.randint(0, C, K).astype(np.int32)
        m = wr.duration_map(n, start, end, n_seg, labels=labels, ratio_q=rq, gap_q=gq, min_frames=int(rng.randint(0, 5)), Fw_max=Fw)
        assert not m.flags & wr.FLAG_TRUNCATED, (n, K, ratio, gap, Fw, m.n_out)
        worst = max(worst, m.n_out - (n * max(int(rq.max()), gq)) // Q)
    assert worst > 0                                                # the rounding term of the bound is needed
    # single frames at rate 1.5 round up one by one: the bound is attained within the rounding term
    n = 9
    start, end = np.arange(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)
    m = wr.duration_map(n, start, end, n, ratio_q=[3 * Q // 2], Fw_max=conversion.duration_max_frames(n, 2 * n + 1, 3 * Q // 2))
    assert m.n_out == 18 and m.flags == 0


def test_time_warp_reference_properties():
    rng = np.random.RandomState(4)
    x = rng.standard_normal((9, 5)).astype(np.float32)
    ident = (np.arange(9) * Q).astype(np.int32)
    assert np.array_equal(wr.time_warp(x, ident, 9, 9), x)
    y = wr.time_warp(x, ident, 6, 9)
    assert np.array_equal(y[:6], x[:6]) and not y[6:].any()
    x[4] = np.nan                                                   # a whole-frame position never touches its neighbour
    assert np.array_equal(wr.time_warp(x, ident, 4, 9)[:4], x[:4])
    ramp = (np.arange(20, dtype=np.float32) * np.float32(2.0 ** -4))[:, None]
    m = wr.duration_map(20, np.array([3]), np.array([17]), 1, ratio_q=[int(1.7 * Q)], gap_q=Q // 2, Fw_max=64)
    got = wr.time_warp(ramp, m.pos, m.n_out, 20)[:m.n_out, 0]
    assert np.array_equal(got, m.pos[:m.n_out].astype(np.float32) * np.float32(2.0 ** -20))
    near = wr.time_warp(ramp, m.pos, m.n_out, 20, mode='nearest')[:m.n_out, 0]
    assert np.array_equal(near * 16, np.minimum((m.pos[:m.n_out].astype(np.int64) + 32768) >> 16, 19))


def test_duration_ratios_on_hand_made_statistics():
    import conversion
    src = (torch.tensor([4, 2, 0, 5, 1, 3]), torch.tensor([40, 10, 0, 50, 8, 0]))          # means 10, 5, -, 10, 8, 0
    tgt = (torch.tensor([2, 2, 3, 1, 1, 3]), torch.tensor([30, 40, 30, 2, 8, 9]))          # means 15, 20, 10, 2, 8, 3
    r = conversion.duration_ratios(src, tgt)
    assert r.dtype == torch.float32 and r.tolist() == [1.5, 2.0, 1.0, 0.5, 1.0, 1.0]        # 4.0 and 0.2 clamped; no source; no frames
    r = conversion.duration_ratios(src, tgt, lo=0.1, hi=8.0, min_count=2)
    assert r.tolist() == [1.5, 4.0, 1.0, 1.0, 1.0, 1.0]                                     # classes 3, 4: one target segment
    with pytest.raises(ValueError):
        conversion.duration_ratios(src, tgt, lo=2.0, hi=1.0)
    # and the statistics themselves, on the host: entries from n_seg on, absent entries and foreign labels are left out
    labels = torch.tensor([[0, 1, 0, 7, 2], [1, -1, 1, 0, 0]])
    start = torch.tensor([[0, 5, 9, 12, 20], [0, -1, 4, 4, 9]])
    end = torch.tensor([[5, 9, 12, 20, 30], [4, -1, 4, 9, 99]])
    st = conversion.duration_stats_batch(labels, start, end, torch.tensor([4, 4]), 3)
    assert st.count.tolist() == [3, 2, 0] and st.total.tolist() == [5 + 3 + 5, 4 + 4, 0]


def test_host_checks_without_gpu():
    import _vc
    import conversion
    s, e = np.array([[0, 10]], np.int32), np.array([[10, 20]], np.int32)
    for kw in (dict(out_len=np.array([[1, 2]]), ratio=[1.0]), dict(labels=np.array([[0, 0]])), dict(ratio=[1.0, 2.0]),
               dict(ratio=[9.0], labels=np.array([[0, 0]])), dict(gap_ratio=-1.0), dict(out_len=np.array([[1, 2]])),
               dict(min_frames=-1), dict(max_frames=0), dict(max_frames=16385)):
        with pytest.raises(ValueError):
            conversion.duration_map_batch(s, e, [2], [30], **kw)
    with pytest.raises(ValueError):
        conversion.duration_map_batch(s, e, [2], [16385])
    assert conversion.duration_min_frames(dict(n_fft=None, win_length=400, hop_length=80)) == 4      # 80 * 3 = 240 > 200
    assert conversion.duration_min_frames(dict(n_fft=512, win_length=400, hop_length=40)) == 8       # 40 * 7 = 280 > 256
    lib = _vc.lib()
    assert lib.vc_duration_map_workspace_bytes(3, 100) == (3 * 101 * 8 + 255) // 256 * 256
    assert lib.vc_duration_map_workspace_bytes(3, 16385) == 0 and lib.vc_duration_map_workspace_bytes(65536, 10) == 0
    # beyond the limits: VC_ERR_UNSUPPORTED before anything is launched (any non-NULL addresses: never dereferenced)
    p = 4096
    args = lambda **k: [p, p, p, None, None, None, 0, k.get('gap_q', Q), p, k.get('batch', 1), k.get('K', 4), k.get('n', 100), 1,
                        k.get('Fw', 100), p, p, p, p, p, p, 1 << 20, None]
    for k in (dict(batch=65536), dict(n=16385), dict(Fw=16385), dict(K=16385), dict(gap_q=8 * Q + 1), dict(gap_q=-1)):
        assert lib.vc_duration_map(*args(**k)) == 4, k
        assert b'vc_duration_map' in lib.vc_last_error()
    assert lib.vc_time_warp(p, p, p, None, 1, 16385, 10, 4, 0, p, None, 0.0, None) == 4
    assert lib.vc_time_warp(p, p, p, None, 1, 10, 10, 4, 2, p, None, 0.0, None) == 1               # an unknown mode
    assert lib.vc_time_warp(p, p, p, None, 1, 10, 10, 4, 0, p, p, 0.0, None) == 1                  # magnitude without a norm factor
