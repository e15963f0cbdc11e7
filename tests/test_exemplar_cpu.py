"""Exemplar conversion without a GPU: the restatement tests/exemplar_ref.py against brute force, the host checks of the three
launchers and of the Python entry points, and the method's own figures on the restatement -- what quantisation costs against
the float64 Hellinger search, and what the retrieved spectrum is worth on the regression corpus and on the vowel corpus
(tests/test_exemplar_gpu.py holds the device to the restatement bit for bit)."""
import ctypes as C

import numpy as np
import pytest

import exemplar_cases as Cs
import exemplar_ref as er
import mapping_cases as mc

VC_ERR_INVALID, VC_ERR_WORKSPACE = 1, 3
P = lambda v=4096: C.c_void_p(v)                        # a non-NULL, 16-byte aligned pointer that no launcher gets to use


def _lib():
    import _vc
    return _vc.lib()


def _refused(rc, text, code=VC_ERR_INVALID):
    msg = _lib().vc_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------------------ restatement
def test_quantiser_edges():
    vals, want = Cs.edge_values()
    key, norm = er.keys(vals[None, :, None])
    got = key[0, :, 0].astype(int).tolist()
    for v, g, w in zip(vals, got, want):
        if w is not None:
            assert g == w, (float(v), g, w)
    assert key.shape == (1, len(vals), 64) and not key[..., 1:].any() and np.array_equal(norm[0], np.array(got) ** 2)
    assert got[list(vals).index(np.float32(0.25))] == 64 and got[list(vals).index(np.float32(0.5))] == 90     # 63.5 -> 64; 89.8 -> 90
    hp = Cs.half_points()
    assert len(hp) >= 20 and {m % 2 for _, m in hp} == {0, 1}, len(hp)            # ties towards both neighbours are present
    for p, m in hp:                                                               # ... and ARE ties in exact arithmetic's eyes
        assert np.float32(127.0) * np.sqrt(p) == np.float32(m + 0.5)


def test_keys_pad_and_mask_rows():
    for c in Cs.KEY_CLASSES:
        p, nf = Cs.key_case(c)
        key, norm = er.keys(p, nf)
        assert key.shape[-1] == er.key_width(c) == (64 if c <= 64 else 128) and key.dtype == np.int8 and norm.dtype == np.int32
        assert key.min() >= 0 and not key[..., c:].any()
        for b, n in enumerate(nf):
            assert not key[b, n:].any() and not norm[b, n:].any()
        assert np.array_equal(norm, (key.astype(np.int64) ** 2).sum(-1))


def test_key_width():
    import exemplar
    assert [exemplar.key_width(c) for c in (1, 61, 64, 65, 128)] == [64, 64, 64, 128, 128]
    assert [_lib().vc_knn_key_width(c) for c in (0, 1, 64, 65, 128, 129)] == [0, 64, 64, 128, 128, 0]
    for c in (0, 129, -1):
        with pytest.raises(ValueError, match='key_width'):
            exemplar.key_width(c)


def test_selection_equals_brute_force_lexsort():
    for seed, (Mq, N, k, keys) in enumerate([(40, 300, 4, Cs.random_keys), (40, 300, 16, Cs.clustered_keys), (7, 5, 8, Cs.clustered_keys)]):
        (qk, qn), (bk, bn) = keys(Mq, 64, seed), keys(N, 64, 100 + seed)
        d = er.distances(qk, qn, bk, bn)
        brute = np.array([[qn[m] + bn[j] - 2 * int(qk[m].astype(np.int64) @ bk[j].astype(np.int64)) for j in range(N)] for m in range(Mq)])
        assert np.array_equal(d, brute) and d.min() >= 0 and d.max() <= Cs.D_MAX
        lo, hi = N // 3, N // 2
        idx, dist = er.select(d, k, lo, hi)
        for m in range(Mq):
            cand = np.array([j for j in range(N) if not lo <= j < hi])
            order = cand[np.lexsort((cand, d[m, cand]))][:k]
            assert idx[m, :len(order)].tolist() == order.tolist() and dist[m, :len(order)].tolist() == d[m, order].tolist()
            assert (idx[m, len(order):] == -1).all() and (dist[m, len(order):] == -1).all()
    assert (np.diff(dist, axis=1) == 0).any()                                     # the clustered banks do tie


def test_extreme_distances():
    full = np.full((1, 128), 127, np.int8)
    zero = np.zeros((1, 128), np.int8)
    n = np.array([Cs.MAX_DOT_128], np.int32)
    assert er.distances(full, n, full, n)[0, 0] == 0 and er.distances(full, n, zero, [0])[0, 0] == Cs.MAX_DOT_128
    assert Cs.MAX_DOT_128 == 2064512 and Cs.D_MAX == 4129024


def test_top_k_of_merged_splits_is_the_global_top_k():
    rng = np.random.RandomState(3)
    (qk, qn), (bk, bn) = Cs.clustered_keys(30, 64, 1), Cs.clustered_keys(500, 64, 2, n_centres=9)
    d = er.distances(qk, qn, bk, bn)
    for k in (1, 4, 16):
        want = er.select(d, k, 100, 140)
        for _ in range(5):
            cuts = np.concatenate([[0], np.sort(rng.randint(0, 501, rng.randint(1, 8))), [500]])       # empty splits happen
            parts = [er.select(d[:, a:b], k, 100, 140, cols=np.arange(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
            got = er.merge(parts, k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_sorted_banks_are_what_they_claim():
    for desc in (False, True):
        q, qn, b, bn = Cs.sorted_bank(100, 64, desc)
        d = er.distances(q, qn, b, bn)[0]
        assert (np.diff(d) < 0).all() if desc else (np.diff(d) > 0).all()


def test_mean_restatement_against_a_loop():
    idx, dist, V = Cs.mean_case(23, 4, 50, 7)
    for d_max in (-1, 0, 2500, 10 ** 6):
        out, n = er.mean(idx, dist, V, d_max)
        for m in range(len(idx)):
            rows = []
            for i in range(4):
                if idx[m, i] < 0 or (i > 0 and d_max >= 0 and dist[m, i] > d_max):
                    break
                rows.append(idx[m, i])
            assert n[m] == len(rows)
            s = np.zeros(7, np.float32)
            for i, r in enumerate(rows):
                s = V[r].copy() if i == 0 else (s + V[r]).astype(np.float32)
            want = (s / np.float32(len(rows))).astype(np.float32) if rows else s
            assert np.array_equal(out[m].view(np.uint32), want.view(np.uint32))


def test_mean_cases_reach_every_gate():
    """The cases of the device test: without a gate and with one above all distances every filled slot counts; d_max = 0 lies
    below every distance, so a filled list counts its first slot alone; d_max = 2500 ends some lists between two slots."""
    for D in Cs.MEAN_DIMS:
        for k in Cs.SEAM_K:
            idx, dist, V = Cs.mean_case(37, k, 50, D)
            filled = (idx >= 0).sum(1)
            assert filled.min() == 0 and filled.max() == k and dist[idx >= 0].min() >= 1
            for d_max in (-1, 10 ** 6):
                assert np.array_equal(er.mean(idx, dist, V, d_max)[1], filled)
            assert np.array_equal(er.mean(idx, dist, V, 0)[1], np.minimum(filled, 1))
            n = er.mean(idx, dist, V, 2500)[1]
            assert (n <= filled).all() and (n >= np.minimum(filled, 1)).all() and (k == 1 or ((n > 1) & (n < filled)).any())


# ---------------------------------------------------------------------------------------------------------- host checks
def test_key_launcher_limits():
    lib = _lib()
    call = lambda ppg=P(), nf=P(), B=2, F=3, c=61, key=P(), norm=P(): lib.vc_ppg_key_i8(ppg, nf, B, F, c, key, norm, None)
    for kw in (dict(ppg=None), dict(nf=None), dict(key=None), dict(norm=None)):
        _refused(call(**kw), 'vc_ppg_key_i8: NULL')
    for c in (0, 129, -5):
        _refused(call(c=c), 'vc_ppg_key_i8: n_classes')
    for kw in (dict(B=0), dict(F=0), dict(B=-1), dict(B=4097, F=4096), dict(B=1 << 20, F=1 << 20)):
        _refused(call(**kw), 'vc_ppg_key_i8: batch')


def test_search_launcher_limits():
    lib = _lib()
    excl = np.array([[0, 0], [2, 5]], np.int32)

    def call(qk=P(), qn=P(), nf=P(), he=None, de=None, B=2, F=3, bk=P(), bn=P(), N=10, Kp=64, k=4, ns=0, ws=P(), wsb=1 << 20, idx=P(), dist=P()):
        he = None if he is None else C.c_void_p(he.ctypes.data)
        return lib.vc_knn_i8(qk, qn, nf, he, de, B, F, bk, bn, N, Kp, k, ns, ws, wsb, idx, dist, None)

    for name in ('qk', 'qn', 'nf', 'bk', 'bn', 'ws', 'idx', 'dist'):
        _refused(call(**{name: None}), 'vc_knn_i8: NULL')
    _refused(call(he=excl), 'vc_knn_i8: pass the exclusion')
    _refused(call(de=P()), 'vc_knn_i8: pass the exclusion')
    for k in (0, 17, -1):
        _refused(call(k=k), 'vc_knn_i8: k must')
    for Kp in (0, 61, 32, 256):
        _refused(call(Kp=Kp), 'vc_knn_i8: key_width')
    for kw in (dict(B=0), dict(F=0), dict(B=4097, F=4096)):
        _refused(call(**kw), 'vc_knn_i8: batch')
    for N in (0, -1, (1 << 24) + 1):
        _refused(call(N=N), 'vc_knn_i8: n_bank')
    for ns in (-1, 1025):
        _refused(call(ns=ns), 'vc_knn_i8: n_splits')
    for name in ('qk', 'bk', 'bn', 'ws'):
        _refused(call(**{name: P(4100)}), 'vc_knn_i8: the keys')
    for bad in ([[0, 0], [5, 2]], [[-1, 3], [0, 0]], [[0, 0], [2, 11]]):
        _refused(call(he=np.array(bad, np.int32), de=P()), 'vc_knn_i8: excl[')
    need = lib.vc_knn_workspace_bytes(6, 10, 4, 0)
    assert need == lib.vc_knn_splits(6, 10, 0) * 6 * 4 * 8 > 0
    _refused(call(wsb=need - 1), 'vc_knn_i8: workspace', VC_ERR_WORKSPACE)


def test_workspace_and_split_queries():
    lib = _lib()
    assert lib.vc_knn_splits(100, 120000, 0) > 64 and 1 < lib.vc_knn_splits(16016, 120000, 0) <= 16       # fills the chip either way
    assert lib.vc_knn_splits(16016, 100, 0) == 1 and lib.vc_knn_splits(5, 1, 7) == 7
    for k, kt in ((1, 1), (2, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16)):
        assert lib.vc_knn_workspace_bytes(33, 1000, k, 3) == 3 * 33 * kt * 8
    for args in ((0, 10, 4, 0), (10, 0, 4, 0), (10, 10, 0, 0), (10, 10, 17, 0), (10, 10, 4, 1025), (10, 10, 4, -1), ((1 << 24) + 1, 10, 4, 0)):
        assert lib.vc_knn_workspace_bytes(*args) == 0, args


def test_mean_launcher_limits():
    lib = _lib()
    call = lambda idx=P(), dist=P(), Mq=5, k=4, d_max=-1, V=P(), N=9, D=80, out=P(), nu=P(): \
        lib.vc_knn_mean_f32(idx, dist, Mq, k, d_max, V, N, D, out, nu, None)
    for name in ('idx', 'dist', 'V', 'out', 'nu'):
        _refused(call(**{name: None}), 'vc_knn_mean_f32: NULL')
    for k in (0, 17):
        _refused(call(k=k), 'vc_knn_mean_f32: k must')
    for Mq in (0, (1 << 24) + 1):
        _refused(call(Mq=Mq), 'vc_knn_mean_f32: n_queries')
    for N in (0, (1 << 24) + 1):
        _refused(call(N=N), 'vc_knn_mean_f32: n_bank')
    for D in (0, 65537):
        _refused(call(D=D), 'vc_knn_mean_f32: dim')


def _bank(N=10, Kp=64, C_=61, bins=201, mels=80):
    import exemplar
    return exemplar.Bank(np.zeros((N, Kp), np.int8), np.zeros((N,), np.int32), np.zeros((N, bins), np.float32),
                         np.zeros((N, mels), np.float32), np.zeros((N,), np.int32), np.zeros((N,), np.int32),
                         np.array([[0, N]], np.int32), C_)


def test_python_checks_raise():
    import exemplar
    ppg = np.full((2, 5, 61), 1.0 / 61, np.float32)
    keys, norms = np.zeros((2, 5, 64), np.int8), np.zeros((2, 5), np.int32)
    bad = [
        lambda: exemplar.ppg_keys(ppg.astype(np.float64), [5, 5]),
        lambda: exemplar.ppg_keys(ppg[0], [5]),
        lambda: exemplar.ppg_keys(np.zeros((2, 5, 129), np.float32), [5, 5]),
        lambda: exemplar.ppg_keys(ppg, [5, 6]),
        lambda: exemplar.ppg_keys(ppg, [5, -1]),
        lambda: exemplar.ppg_keys(ppg, [5]),
        lambda: exemplar.build_bank(ppg, [5, 5], np.zeros((2, 5, 201)), np.zeros((2, 5, 80), np.float32)),
        lambda: exemplar.build_bank(ppg, [5, 5], np.zeros((2, 4, 201), np.float32), np.zeros((2, 5, 80), np.float32)),
        lambda: exemplar.build_bank(ppg, [5, 5], np.zeros((2, 5, 201), np.float32), np.zeros((2, 5, 80), np.float32), mask=np.ones((2, 4))),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], (1, 2)),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(Kp=128)),
        lambda: exemplar.knn_batch(keys.astype(np.int32), norms, [5, 5], _bank()),
        lambda: exemplar.knn_batch(keys, norms[:, :4], [5, 5], _bank()),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), k=0),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), k=17),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), k=2.5),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), n_splits=-1),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), n_splits=1025),
        lambda: exemplar.knn_batch(keys, norms, [5, 7], _bank()),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), exclude=[[0, 11], [0, 0]]),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), exclude=[[3, 2], [0, 0]]),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank(), exclude=[[0, 1]]),
        lambda: exemplar.knn_batch(keys, norms, [5, 5], _bank()._replace(norm=np.zeros((9,), np.int32))),
        lambda: exemplar.mean_batch(np.zeros((2, 5, 4), np.int64), np.zeros((2, 5, 4), np.int32), np.zeros((9, 3), np.float32)),
        lambda: exemplar.mean_batch(np.zeros((2, 5, 4), np.int32), np.zeros((2, 5, 3), np.int32), np.zeros((9, 3), np.float32)),
        lambda: exemplar.mean_batch(np.zeros((2, 5, 17), np.int32), np.zeros((2, 5, 17), np.int32), np.zeros((9, 3), np.float32)),
        lambda: exemplar.mean_batch(np.zeros((2, 5, 4), np.int32), np.zeros((2, 5, 4), np.int32), np.zeros((9, 3), np.float64)),
        lambda: exemplar.mean_batch(np.zeros((2, 5, 4), np.int32), np.zeros((2, 5, 4), np.int32), np.zeros((9,), np.float32)),
        lambda: exemplar.mean_batch(np.zeros((2, 5, 4), np.int32), np.zeros((2, 5, 4), np.int32), np.zeros((9, 3), np.float32), d_max=-3),
        lambda: exemplar.mean_batch(np.zeros((2, 5, 4), np.int32), np.zeros((2, 5, 4), np.int32), np.zeros((9, 3), np.float32), d_max=0.5),
        lambda: exemplar.bank_wav(None, np.zeros((1, 16000), np.float32), None, mc.CFG),
        lambda: exemplar.bank_wav(None, np.zeros((1, 16000), np.float32), None, None, ppg=ppg),
        lambda: exemplar.bank_wav(None, np.zeros((1, 16000), np.float32), None, mc.CFG, ppg=ppg, mask='voiced'),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError, match=' - ERROR, '):
            f()
            pytest.fail('case %d did not raise' % i)


def test_convert_knn_diff_checks_raise():
    import conversion
    cfg = dict(mc.CFG, n_timesteps=40)
    wav = np.zeros((2, 8000), np.float32)
    F = conversion.convert_plan([8000, 8000], cfg, 0, 60, True).Fout
    ppg = np.full((2, F, 61), 1.0 / 61, np.float32)
    ok = dict(bank=_bank(), wav=wav, cfg_d=cfg, ppg=ppg)
    bad = [dict(ppg=None), dict(encoder=object()), dict(cfg_d=None), dict(k=0), dict(k=17), dict(d_max=-2), dict(n_splits=2000),
           dict(bank=(1, 2, 3)), dict(bank=_bank(C_=60)), dict(bank=_bank(bins=200)), dict(bank=_bank(mels=40)),
           dict(ppg=ppg[:, :-1]), dict(ppg=ppg[..., :60]), dict(exclude=[[0, 11], [0, 0]]), dict(exclude=[[4, 2], [0, 0]]),
           dict(alpha=-1.0), dict(half_width=99), dict(pitch='source'), dict(lens=[8000, 100]), dict(wav=wav[0])]
    for kw in bad:
        with pytest.raises(ValueError, match=' - ERROR, '):
            conversion.convert_knn_diff_batch(**dict(ok, **kw))
            pytest.fail('%r did not raise' % (kw,))


# -------------------------------------------------------------------------------------------------- the method's figures
def test_quantisation_against_the_float64_hellinger_search():
    """61 classes, 2,000 queries against 20,000 bank frames, k = 8: the float64 nearest neighbour is inside the quantised
    first 8 for at least 99 % of the queries, and the mean float64 Hellinger^2 of the neighbours chosen lies within 1 % of the
    exact search's.  Ties inside the first 9 are common, so the tie rule is not academic."""
    contained, h_q, h_x, tied = er.fidelity()
    print('\nMEASURED containment=%.4f mean Hellinger^2 quantised=%.5f exact=%.5f ties=%.3f' % (contained, h_q, h_x, tied))
    assert contained >= 0.99
    assert h_x <= h_q <= 1.01 * h_x
    assert tied > 0.01


@pytest.mark.parametrize('noise', [0.02, 0.3])
def test_regression_corpus(noise):
    """21 classes, an envelope per class and speaker, a bank of 16 target utterances, k = 4: the retrieved spectrum's rms
    error to the target's trajectory is at most half the source's own."""
    c = er.regression_corpus(noise)
    got, src, idx, dist, _ = er.regression_figures(c)
    print('\nMEASURED noise=%.2f bank=%d frames retrieved rms=%.4f source rms=%.4f ratio=%.3f'
          % (noise, sum(len(p) for p in c['bank_ppg']), got, src, got / src))
    assert got <= 0.5 * src
    assert (idx >= 0).all() and (np.diff(dist, axis=1) >= 0).all()


def test_vowel_corpus_restatement():
    """The whole conversion in numpy on the vowel corpus: the filtered source's smoothed log-spectral distance to the target
    speaker's rendition is at most half the source's."""
    y, d_src, d_out, _ = er.vowel_restatement(er.vowel_corpus(), mc.CFG)
    print('\nMEASURED vowel corpus: log-spectral distance to the target %.3f dB -> %.3f dB' % (d_src, d_out))
    assert np.isfinite(y).all() and d_out <= 0.5 * d_src
