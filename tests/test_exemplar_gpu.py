"""Exemplar conversion on the device: vc_ppg_key_i8, vc_knn_i8 and vc_knn_mean_f32 of csrc/vc_knn.hip alone, through the C
ABI with raw pointers, and conversion.convert_knn_diff_batch -- all bit for bit against tests/exemplar_ref.py on the cases of
tests/exemplar_cases.py (tests/test_exemplar_cpu.py proves those usable).

The memory contract of the kernel tests: every output and the workspace lie between two bands of sentinels that are checked
after each call; the workspace is exactly as long as the size query says; outputs start as sentinels and none may be left;
inputs hold NaN (the key 0x7f, a huge norm) in the rows at or beyond an utterance's frame count."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import exemplar_cases as Cs
import exemplar_ref as er
import mapping_cases as mc

pytestmark = pytest.mark.gpu

BAND, CAN = 256, 0xA5


def _lib():
    import _vc
    return _vc.lib()


def _st():
    import _vc
    return _vc.current_stream()


def _ok(rc):
    import _vc
    _vc.check(rc)
    torch.cuda.synchronize()


class Buf:
    """nbytes between two bands of sentinel bytes; the body starts 16-byte aligned."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + 2 * BAND,), CAN, dtype=torch.uint8, device='cuda')
        assert self.raw.data_ptr() % 16 == 0

    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + BAND)

    def read(self, dtype, shape, written=True):
        torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        assert (raw[:BAND] == CAN).all() and (raw[BAND + self.n:] == CAN).all(), 'wrote outside the buffer'
        body = raw[BAND:BAND + self.n].copy().view(dtype)
        if written and np.dtype(dtype).itemsize == 4:
            assert not (body.view(np.uint32) == 0xA5A5A5A5).any(), 'elements were never written'
        return body.reshape(shape)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_keys(ppg, nf):
    B, F, c = ppg.shape
    Kp = er.key_width(c)
    key, norm = Buf(B * F * Kp), Buf(B * F * 4)
    d_p, d_n = dev(ppg), dev(np.asarray(nf, np.int32))
    _ok(_lib().vc_ppg_key_i8(ptr(d_p), ptr(d_n), B, F, c, key.ptr(), norm.ptr(), _st()))
    k = key.read(np.int8, (B, F, Kp), written=False)
    assert not (k.view(np.uint8) == CAN).any()                               # 0xA5 is no key: every byte was written
    return k, norm.read(np.int32, (B, F))


def run_knn(qk, qn, nf, bk, bn, k, excl=None, n_splits=0):
    """qk [B, F, Kp], qn [B, F], nf [B]; bank bk [N, Kp], bn [N]; excl None or [B, 2].  Returns idx, dist [B, F, k]."""
    lib = _lib()
    B, F, Kp = qk.shape
    N = len(bk)
    need = lib.vc_knn_workspace_bytes(B * F, N, k, n_splits)
    assert need > 0
    ws, idx, dist = Buf(need), Buf(B * F * k * 4), Buf(B * F * k * 4)
    d = [dev(a) for a in (qk, qn, np.asarray(nf, np.int32), bk, bn)]
    h_e = None if excl is None else np.ascontiguousarray(excl, np.int32)
    d_e = None if excl is None else dev(h_e)
    _ok(lib.vc_knn_i8(ptr(d[0]), ptr(d[1]), ptr(d[2]), None if h_e is None else C.c_void_p(h_e.ctypes.data), ptr(d_e), B, F, ptr(d[3]),
                      ptr(d[4]), N, Kp, k, n_splits, ws.ptr(), need, idx.ptr(), dist.ptr(), _st()))
    ws.read(np.uint8, (need,))
    return idx.read(np.int32, (B, F, k)), dist.read(np.int32, (B, F, k))


def run_mean(idx, dist, V, d_max):
    Mq, k = idx.shape
    N, D = V.shape
    out, nu = Buf(Mq * D * 4), Buf(Mq * 4)
    d = [dev(a) for a in (idx, dist, V)]
    _ok(_lib().vc_knn_mean_f32(ptr(d[0]), ptr(d[1]), Mq, k, d_max, ptr(d[2]), N, D, out.ptr(), nu.ptr(), _st()))
    return out.read(np.uint32, (Mq, D)), nu.read(np.int32, (Mq,))


def same(got, want, what):
    for g, w, name in zip(got, want, ('idx', 'dist')):
        assert np.array_equal(g, w), '%s: %s differs in %d of %d places' % (what, name, int((g != w).sum()), g.size)


def dirty(qk, qn, nf):
    """Garbage in the query rows at or beyond the frame counts."""
    qk, qn = qk.copy(), qn.copy()
    for b, n in enumerate(nf):
        qk[b, n:], qn[b, n:] = 0x7F, 0x7FFFFFF
    return qk, qn


# ------------------------------------------------------------------------------------------------------------------- keys
@pytest.mark.parametrize('c', Cs.KEY_CLASSES)
def test_keys(c):
    ppg, nf = Cs.key_case(c)
    got = run_keys(ppg, nf)
    want = er.keys(ppg, nf)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_key_edge_values():
    vals, want = Cs.edge_values()
    got, norm = run_keys(vals[None, :, None], [len(vals)])
    ref, _ = er.keys(vals[None, :, None])
    assert np.array_equal(got, ref)
    for v, g, w in zip(vals, got[0, :, 0], want):
        assert w is None or g == w, (float(v), int(g), w)


# ----------------------------------------------------------------------------------------------------------------- search
@pytest.mark.parametrize('Kp', [64, 128])
def test_search_operand_maps(Kp):
    """Random asymmetric keys over 0 .. 127: a lane map that swapped rows, columns or K chunks between the operands would not
    survive.  At Kp = 128 the all-127 key and the zero key sit among queries and bank: dot 2,064,512 and distance 4,129,024."""
    qk, qn = Cs.random_keys(40, Kp, 1)
    bk, bn = Cs.random_keys(203, Kp, 2)
    for keys, norms in ((qk, qn), (bk, bn)):
        keys[3], keys[5] = 127, 0
        norms[3], norms[5] = Kp * 127 * 127, 0
    want = er.knn(qk[None], qn[None], [40], bk, bn, 16)
    assert want[1][0, 3, 0] == 0 and want[0][0, 3, 0] == 3 and want[1][0, 5, 0] == 0 and want[0][0, 5, 0] == 5
    d = er.distances(qk, qn, bk, bn)
    assert d[3, 5] == Kp * 127 * 127 == d[5, 3] and (Kp == 64 or d[3, 5] == Cs.MAX_DOT_128)
    same(run_knn(qk[None], qn[None], [40], bk, bn, 16), want, 'Kp %d' % Kp)
    # the farthest pair must be reported too: a bank of the zero key and the full key alone
    two_k, two_n = np.stack([bk[5], bk[3]]), np.array([0, Kp * 127 * 127], np.int32)
    got = run_knn(qk[None, 3:4], qn[None, 3:4], [1], two_k, two_n, 2)
    assert got[0][0, 0].tolist() == [1, 0] and got[1][0, 0].tolist() == [0, Kp * 127 * 127]


@pytest.mark.parametrize('N', Cs.SEAM_N)
def test_search_seams(N):
    """Query counts and bank sizes around the 16-row tiles, k = 1, 4, 16, every split count: identical bits for all of them
    (splits beyond the bank's tiles are empty)."""
    bk, bn = Cs.clustered_keys(N, 64, 7 + N, n_centres=11) if N % 2 else Cs.random_keys(N, 64, 7 + N, C=61)
    for Mq in Cs.SEAM_MQ:
        qk, qn = Cs.random_keys(Mq, 64, 100 + Mq, C=61)
        for k in Cs.SEAM_K:
            want = er.knn(qk[None], qn[None], [Mq], bk, bn, k)
            for ns in Cs.SEAM_SPLITS:
                same(run_knn(qk[None], qn[None], [Mq], bk, bn, k, n_splits=ns), want, 'Mq %d N %d k %d splits %d' % (Mq, N, k, ns))


def test_search_banks_smaller_than_k():
    qk, qn = Cs.random_keys(17, 128, 3)
    for k in Cs.SEAM_K:
        for N in sorted({max(1, k - 1), k, k + 1}):
            bk, bn = Cs.random_keys(N, 128, 40 + N)
            want = er.knn(qk[None], qn[None], [17], bk, bn, k)
            assert (want[0][..., min(N, k):] == -1).all() and (want[0][..., :min(N, k)] >= 0).all()
            for ns in (1, 3, 0):
                same(run_knn(qk[None], qn[None], [17], bk, bn, k, n_splits=ns), want, 'k %d N %d splits %d' % (k, N, ns))


def test_search_ties():
    """All bank rows equal: idx must be 0 .. k - 1.  Duplicated rows across a tile seam (rows 15, 16) and across a split seam
    (64 rows in two splits: rows 31, 32): the lower row first."""
    qk, qn = Cs.random_keys(5, 64, 9)
    one_k, one_n = Cs.random_keys(1, 64, 10)
    bk, bn = np.repeat(one_k, 100, 0), np.repeat(one_n, 100)
    for k in Cs.SEAM_K:
        for ns in (1, 2, 5):
            idx, dist = run_knn(qk[None], qn[None], [5], bk, bn, k, n_splits=ns)
            assert (idx[0] == np.arange(k)[None, :]).all() and (dist[0] == dist[0][:, :1]).all()
    bk, bn = Cs.random_keys(64, 64, 11)
    bk[:] = np.maximum(bk, 1)                                                  # far from the query, which is row 15's copy
    bn = (bk.astype(np.int32) ** 2).sum(1).astype(np.int32)
    for a, b in ((15, 16), (31, 32)):
        k2, n2 = bk.copy(), bn.copy()
        k2[b], n2[b] = k2[a], n2[a]
        q, qn1 = k2[a][None, None], n2[a][None, None]
        want = er.knn(q, qn1, [1], k2, n2, 4)
        assert want[0][0, 0, :2].tolist() == [a, b] and want[1][0, 0, :2].tolist() == [0, 0]
        for ns in (1, 2):
            same(run_knn(q, qn1, [1], k2, n2, 4, n_splits=ns), want, 'duplicates %d %d splits %d' % (a, b, ns))


@pytest.mark.parametrize('descending', [False, True])
def test_search_insertion_paths(descending):
    """A bank sorted by ascending distance (after the first k nothing inserts) and by descending distance (every candidate
    inserts at the front)."""
    q, qn, bk, bn = Cs.sorted_bank(100, 64, descending)
    for k in Cs.SEAM_K:
        want = er.knn(q[None], qn[None], [1], bk, bn, k)
        rows = np.arange(100)[::-1][:k] if descending else np.arange(k)
        assert want[0][0, 0].tolist() == rows.tolist()
        for ns in (1, 3):
            same(run_knn(q[None], qn[None], [1], bk, bn, k, n_splits=ns), want, 'k %d splits %d' % (k, ns))


def test_search_exclusion():
    """96 bank rows = 6 tiles (splits of 3: seams at rows 32 and 64): ranges that start or end at tile and split seams, one
    row off them, the whole bank, nothing."""
    qk, qn = Cs.random_keys(18, 64, 21)
    bk, bn = Cs.clustered_keys(96, 64, 22, n_centres=7)
    for lo, hi in ((0, 0), (16, 32), (15, 33), (17, 31), (0, 16), (80, 96), (32, 64), (31, 65), (33, 63), (0, 96), (1, 96), (0, 95), (40, 40)):
        for k in (4, 16):
            want = er.knn(qk[None], qn[None], [18], bk, bn, k, excl=[(lo, hi)])
            assert not ((want[0] >= lo) & (want[0] < hi)).any()
            if (lo, hi) == (0, 96):
                assert (want[0] == -1).all() and (want[1] == -1).all()
            for ns in (1, 2, 3):
                same(run_knn(qk[None], qn[None], [18], bk, bn, k, excl=[(lo, hi)], n_splits=ns), want, 'excl %d %d k %d splits %d' % (lo, hi, k, ns))


def test_search_rows_and_batch():
    """A batch whose utterances have different frame counts (one of them 0) and different exclusions; the rows beyond a count
    hold garbage keys and come back as -1."""
    B, F, nf = 4, 21, [21, 0, 7, 16]
    excl = [(0, 0), (3, 9), (10, 50), (0, 64)]
    qk, qn = Cs.random_keys(B * F, 64, 31, C=61)
    qk, qn = dirty(qk.reshape(B, F, 64), qn.reshape(B, F), nf)
    bk, bn = Cs.random_keys(70, 64, 32, C=61)
    want = er.knn(qk, qn, nf, bk, bn, 4, excl=excl)
    for b, n in enumerate(nf):
        assert (want[0][b, n:] == -1).all() and (want[0][b, :n] >= 0).all()
    for ns in (0, 1, 2):
        same(run_knn(qk, qn, nf, bk, bn, 4, excl=excl, n_splits=ns), want, 'splits %d' % ns)
    same(run_knn(qk, qn, nf, bk, bn, 4), er.knn(qk, qn, nf, bk, bn, 4), 'no table')


# ------------------------------------------------------------------------------------------------------------------- mean
@pytest.mark.parametrize('D', Cs.MEAN_DIMS)
def test_mean(D):
    """Lists with -1 tails of every length (none filled: zeros and n_used 0), d_max below the first distance (n = 1), between
    slots, above all, and absent."""
    for k in Cs.SEAM_K:
        idx, dist, V = Cs.mean_case(37, k, 50, D)
        for d_max in (-1, 0, 2500, 10 ** 6):
            out, n = er.mean(idx, dist, V, d_max)
            got, got_n = run_mean(idx, dist, V, d_max)
            assert np.array_equal(got_n, n), (k, d_max)
            assert np.array_equal(got, out.view(np.uint32)), (k, d_max)
            assert n[0] == 0 and not got[0].any()                              # (tests/test_exemplar_cpu.py: what each d_max cuts)
    # an index beyond the bank ends the list like -1
    idx, dist, V = Cs.mean_case(5, 4, 50, D)
    idx[4] = [3, 50, 2, 1]
    got, got_n = run_mean(idx, dist, V, -1)
    assert got_n[4] == 1 and np.array_equal(got[4], V[3].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ graph
def test_graph_replay_of_the_chain():
    """Key, search and mean captured once and replayed on new posteriors: bit-identical to eager calls and to the
    restatement."""
    import exemplar
    from test_graph_replay_gpu import _capture, _free, _same
    rng = np.random.RandomState(0)
    B, F, c, nf = 2, 40, 61, [40, 23]
    bank_p = er.peaky_posteriors(300, c, seed=5)
    bk, bn = exemplar.ppg_keys(bank_p[None], [300])
    V = dev(rng.standard_normal((300, 80)).astype(np.float32))
    bank = exemplar.Bank(bk[0], bn[0], V, V, None, None, None, c)
    d_nf = dev(np.array(nf, np.int32))
    ws = torch.empty((exemplar.workspace_bytes(B * F, 300, 4),), dtype=torch.uint8, device='cuda')

    def chain(ppg):
        key, norm = exemplar._key_launch(ppg, d_nf)
        idx, dist = exemplar._knn_launch(key, norm, d_nf, None, None, bank, 4, 0, ws)
        return (key, norm, idx, dist) + exemplar._mean_launch(idx, dist, V, -1)

    inputs = [dev(er.peaky_posteriors(B * F, c, seed=10 + i).reshape(B, F, c)) for i in range(3)]
    static = inputs[0].clone()
    g, outs = _capture(lambda: chain(static))
    try:
        for i in (1, 2):
            static.copy_(inputs[i])
            g.replay()
            torch.cuda.synchronize()
            for j, (a, b) in enumerate(zip(outs, chain(inputs[i]))):
                _same(a, b, 'replay %d output %d' % (i, j))
            hk, hn = er.keys(inputs[i].cpu().numpy(), nf)
            want = er.knn(hk, hn, nf, bk[0].cpu().numpy(), bn[0].cpu().numpy(), 4)
            assert np.array_equal(outs[2].cpu().numpy(), want[0]) and np.array_equal(outs[3].cpu().numpy(), want[1])
    finally:
        _free(g)


# ------------------------------------------------------------------------------------------------------------- end to end
CFG = dict(mc.CFG, n_timesteps=40)


def _pad_ppg(ps, F):
    out = np.full((len(ps), F, ps[0].shape[1]), np.nan, np.float32)        # (rows at or beyond the frame count are not read)
    for b, p in enumerate(ps):
        out[b, :len(p)] = p[:F]
    return out


def _normalise(y, d_nf, c):
    import audio_lib
    import _vc
    y = y.clone()
    vplan = audio_lib._get_voc_plan(c['win_length'], c['hop_length'], c['n_fft'])
    _vc.check(_vc.lib().vc_inv_preemphasis_normalize(vplan.handle, _vc.ptr(y), _vc.ptr(d_nf), y.shape[0], 1 + y.shape[1] // c['hop_length'],
                                                     y.shape[1], 0.0, float(15 * c['mean_abs_amp_norm']), _vc.current_stream()))
    return y


def _by_hand(r, bank, wav, lens, c, k, d_max=None, exclude=None):
    """The stages behind the posteriors composed from the public calls; asserts every field of r equal bit for bit."""
    import audio_lib
    import conversion
    import exemplar
    nf = r.n_frames
    keys, norms = exemplar.ppg_keys(r.phn_pred, nf)
    idx, dist = exemplar.knn_batch(keys, norms, nf, bank, k=k, exclude=exclude)
    stft_pred, n_used = exemplar.mean_batch(idx, dist, bank.stft, d_max)
    mel_pred, _ = exemplar.mean_batch(idx, dist, bank.mel, d_max)
    for name, t in (('idx', idx), ('dist', dist), ('n_used', n_used), ('stft_pred', stft_pred), ('mel_pred', mel_pred)):
        assert torch.equal(getattr(r, name), t), name
    d_nf = torch.tensor(nf, dtype=torch.int32, device='cuda')
    gain = conversion.diff_gain_batch(stft_pred, r.stft_true, d_nf, c['P_dB_norm_factor'])
    assert torch.equal(r.gain, gain)
    y = audio_lib.stft_filter_batch(wav, lens, gain, d_nf, c['win_length'], c['hop_length'], c['n_fft'])
    assert torch.equal(r.y_wav_pred, _normalise(y, d_nf, c))
    return keys, norms


def test_convert_knn_diff_with_ppg_on_the_vowel_corpus():
    """The vowel corpus of tests/exemplar_ref.py, posteriors from the known segmentation: the output equals the stages composed
    by hand bit for bit, the retrieval equals the restatement on the device's own spectra bit for bit, and the filtered
    source's smoothed log-spectral distance to the target speaker's rendition is at most half the source's.
    Measured: restatement 5.564 dB -> 0.950 dB (tests/test_exemplar_cpu.py); the device's figure is printed
    (profiles/knn/README.md records both)."""
    import conversion
    import exemplar
    import diff_ref
    import mapping_ref as mr
    import vocoder_kernels_ref as vr
    v = er.vowel_corpus()
    hop = CFG['hop_length']
    bw, bl = mr.wav_batch(v['bank_wav'])
    plan = conversion.convert_plan(bl, CFG, 0, 60, True)
    bank = exemplar.bank_wav(None, bw, bl, CFG, mask=None, ppg=_pad_ppg(v['bank_ppg'], plan.Fout))
    n_bank = [1 + n // hop for n in bl]
    assert bank.rows.tolist() == np.stack([np.cumsum([0] + n_bank[:-1]), np.cumsum(n_bank)], 1).tolist() and bank.n_classes == er.VOWEL_CLASSES
    hk, hn = er.keys(np.concatenate(v['bank_ppg']))
    assert np.array_equal(bank.key.cpu().numpy(), hk) and np.array_equal(bank.norm.cpu().numpy(), hn)
    src, n = v['src'][None], len(v['src'])
    Fout = conversion.convert_plan([n], CFG, 0, 60, True).Fout
    ppg = _pad_ppg([v['src_ppg']], Fout)
    r = conversion.convert_knn_diff_batch(bank, src, [n], CFG, ppg=ppg, k=4)
    F = 1 + n // hop
    assert r.n_frames == [F] and [int(x) for x in r.n_samples] == [hop * (F - 1)]
    _by_hand(r, bank, src, [n], CFG, 4)
    # the retrieval against the restatement, on the device's spectra
    qk, qn = er.keys(v['src_ppg'][None], [F])
    want = er.knn(qk, qn, [F], hk, hn, 4)
    idx, dist = r.idx.cpu().numpy(), r.dist.cpu().numpy()
    assert np.array_equal(idx[:, :F], want[0]) and np.array_equal(dist[:, :F], want[1]) and (idx[:, F:] == -1).all()
    out, _ = er.mean(want[0][0], want[1][0], bank.stft.cpu().numpy())
    got = r.stft_pred[0].cpu().numpy()
    assert np.array_equal(got[:F].view(np.uint32), out.view(np.uint32)) and not got[F:].any()
    # what it is worth
    y = r.y_wav_pred[0, :hop * (F - 1)].cpu().numpy().astype(np.float64)
    win, taps = vr.device_window(vr.padded_window(CFG['win_length'], CFG['win_length'])), diff_ref.smoothing_taps(8)
    lsd = lambda a: diff_ref.log_spectral_distance(a[:len(y)], v['tgt'][:len(y)].astype(np.float64), win, hop, taps)
    d_src, d_out = lsd(v['src'].astype(np.float64)), lsd(y)
    print('\nMEASURED vowel corpus on the device: log-spectral distance to the target %.3f dB -> %.3f dB' % (d_src, d_out))
    assert np.isfinite(y).all() and d_out <= 0.5 * d_src


@pytest.fixture(scope='module')
def golden_encoder(golden_dir):
    from encoder import encoder_spec_phn
    from test_conversion_gpu import _cfgs
    enc_cfg, _, c = _cfgs(golden_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(enc_cfg, None)
    return enc, c


def test_convert_knn_diff_with_the_golden_encoder(golden_encoder):
    """Synthetic speech through the shipped recogniser.  The output equals the hand composition bit for bit.  With the bank
    built from the same recordings without a mask and k = 1 every valid frame finds a key equal to its own at distance 0;
    where the nearest row is the frame's own (always, unless an EARLIER bank frame carries the same key: the (d, j) order
    then returns that one) stft_pred is stft_true bit for bit.  With exclude=bank.rows no index falls inside the excluded
    range.  Nothing is asserted about what the recogniser makes of synthetic audio -- measured: it puts all its mass on one
    class, so all 742 frames carry ONE key and 741 of them retrieve row 0; "stft_pred == stft_true on every valid frame"
    holds only where keys are distinct, and test_self_retrieval_with_distinct_keys asserts it there, on every frame."""
    import conversion
    import evaluation
    import exemplar
    from oracle import frontend_oracle as fo
    enc, c = golden_encoder
    lens = [int(1.5 * 16000), int(2.2 * 16000)]
    wav = np.zeros((2, max(lens)), np.float32)
    for b, L in enumerate(lens):
        wav[b, :L] = fo.synth_speech(1, L, seed=21 + b)[0]
    bank = exemplar.bank_wav(enc, wav, lens, c, mask=None, window_batch=4)
    r = conversion.convert_knn_diff_batch(bank, wav, lens, c, encoder=enc, k=1, window_batch=4)
    nf = r.n_frames
    assert nf == [1 + L // c['hop_length'] for L in lens] and bank.rows.tolist() == [[0, nf[0]], [nf[0], nf[0] + nf[1]]]
    ppg = evaluation.content_wav_batch(enc, wav, lens, wav, lens, c, window_batch=4).ppg_a
    assert torch.equal(r.phn_pred, ppg)
    keys, norms = _by_hand(r, bank, wav, lens, c, 1)
    idx, dist = r.idx.cpu().numpy()[..., 0], r.dist.cpu().numpy()[..., 0]
    bkey, keys = bank.key.cpu().numpy(), keys.cpu().numpy()
    stft_pred, stft_true = r.stft_pred.cpu().numpy(), r.stft_true.cpu().numpy()
    own = 0
    for b, n in enumerate(nf):
        assert (dist[b, :n] == 0).all() and (idx[b, n:] == -1).all()
        assert np.array_equal(bkey[idx[b, :n]], keys[b, :n])
        mine = bank.rows[b, 0] + np.arange(n)
        assert (idx[b, :n] <= mine).all()
        for f in np.nonzero(idx[b, :n] < mine)[0]:                             # an earlier frame with the same key
            assert np.array_equal(bkey[idx[b, f]], bkey[mine[f]])
        at = idx[b, :n] == mine
        own += int(at.sum())
        assert np.array_equal(stft_pred[b, :n][at].view(np.uint32), stft_true[b, :n][at].view(np.uint32))
    print('\nMEASURED golden encoder, k = 1: %d of %d frames retrieve themselves, the rest an earlier frame with an identical key'
          % (own, sum(nf)))
    assert own > 0
    x = conversion.convert_knn_diff_batch(bank, wav, lens, c, encoder=enc, k=4, exclude=bank.rows, window_batch=4)
    _by_hand(x, bank, wav, lens, c, 4, exclude=bank.rows)
    xi = x.idx.cpu().numpy()
    for b, n in enumerate(nf):
        lo, hi = bank.rows[b]
        assert (xi[b, :n] >= 0).all() and not ((xi[b, :n] >= lo) & (xi[b, :n] < hi)).any()


def test_self_retrieval_with_distinct_keys():
    """The bank built from the very recordings that are converted (vowel corpus, posteriors from the segmentation, no mask),
    k = 1: dist 0 on every valid frame, the key found is the query's, and wherever no earlier bank row carries the same key
    -- asserted to be at least nine frames in ten -- the frame retrieves itself and stft_pred is stft_true bit for bit."""
    import conversion
    import exemplar
    import mapping_ref as mr
    v = er.vowel_corpus()
    bw, bl = mr.wav_batch(v['bank_wav'])
    ppg = _pad_ppg(v['bank_ppg'], conversion.convert_plan(bl, CFG, 0, 60, True).Fout)
    bank = exemplar.bank_wav(None, bw, bl, CFG, mask=None, ppg=ppg)
    r = conversion.convert_knn_diff_batch(bank, bw, bl, CFG, ppg=ppg, k=1)
    bkey = bank.key.cpu().numpy()
    _, first = np.unique(bkey, axis=0, return_index=True)
    is_first = np.zeros(len(bkey), bool)
    is_first[first] = True                                                    # no earlier row with this key
    idx, dist = r.idx.cpu().numpy()[..., 0], r.dist.cpu().numpy()[..., 0]
    pred, true = r.stft_pred.cpu().numpy(), r.stft_true.cpu().numpy()
    assert is_first.mean() >= 0.9, is_first.mean()
    for b, n in enumerate(r.n_frames):
        mine = bank.rows[b, 0] + np.arange(n)
        assert (dist[b, :n] == 0).all() and np.array_equal(bkey[idx[b, :n]], bkey[mine])
        u = is_first[mine]
        assert np.array_equal(idx[b, :n][u], mine[u])
        assert np.array_equal(pred[b, :n][u].view(np.uint32), true[b, :n][u].view(np.uint32))
    x = conversion.convert_knn_diff_batch(bank, bw, bl, CFG, ppg=ppg, k=4, exclude=bank.rows)
    xi = x.idx.cpu().numpy()
    for b, n in enumerate(x.n_frames):
        assert (xi[b, :n] >= 0).all() and not ((xi[b, :n] >= bank.rows[b, 0]) & (xi[b, :n] < bank.rows[b, 1])).any()


def test_bank_wav_masks_silence():
    """Two vowel sentences with 0.4 s of digital silence between them: the masked bank is the unmasked one compacted by
    evaluation.activity_batch's energy mask."""
    import conversion
    import evaluation
    import exemplar
    import mapping_ref as mr
    v = er.vowel_corpus(n_bank=2)
    w = np.concatenate([v['bank_wav'][0], np.zeros(6400, np.float32), v['bank_wav'][1]])
    bw, bl = mr.wav_batch([w, v['bank_wav'][1]])
    Fout = conversion.convert_plan(bl, CFG, 0, 60, True).Fout
    ppg = er.peaky_posteriors(2 * Fout, 61, seed=3).reshape(2, Fout, 61)
    full = exemplar.bank_wav(None, bw, bl, CFG, mask=None, ppg=ppg)
    masked = exemplar.bank_wav(None, bw, bl, CFG, mask='energy', ppg=ppg)
    m = evaluation.activity_batch(bw, bl, hop_length=CFG['hop_length'], frame_length=CFG['win_length']).mask.cpu().numpy()
    nf = [1 + n // CFG['hop_length'] for n in bl]
    keep = np.concatenate([m[b, :nf[b]] != 0 for b in range(2)])
    assert 0 < keep.sum() < len(keep) - 40 and len(keep) == full.key.shape[0] and masked.key.shape[0] == keep.sum()
    for name in ('key', 'norm', 'stft', 'mel', 'utt', 'frame'):
        assert torch.equal(getattr(masked, name), getattr(full, name)[torch.from_numpy(keep).cuda()]), name
    assert masked.rows.tolist() == [[0, int(keep[:nf[0]].sum())], [int(keep[:nf[0]].sum()), int(keep.sum())]]


def test_no_host_synchronisation_inside_the_calls():
    import conversion
    import exemplar
    import mapping_ref as mr
    v = er.vowel_corpus(n_bank=2)
    bw, bl = mr.wav_batch(v['bank_wav'])
    bank = exemplar.bank_wav(None, bw, bl, CFG, mask=None, ppg=_pad_ppg(v['bank_ppg'], conversion.convert_plan(bl, CFG, 0, 60, True).Fout))
    n = len(v['src'])
    src = torch.from_numpy(v['src'][None]).cuda()                              # (one row: its stride is arbitrary)
    ppg = torch.from_numpy(np.nan_to_num(_pad_ppg([v['src_ppg']], conversion.convert_plan([n], CFG, 0, 60, True).Fout))).cuda()
    call = lambda: conversion.convert_knn_diff_batch(bank, src, [n], CFG, ppg=ppg, k=4, exclude=[0, 10])
    call()                                                                      # warm-up: plans, tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = call()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(r.y_wav_pred).all()
