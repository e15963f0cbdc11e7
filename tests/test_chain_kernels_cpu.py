"""What tests/test_chain_kernels_gpu.py relies on, proven without a device: tests/chain_ref.py against the oracle and against
torch's bf16 conversion, its pack formulas against the host code's arrangement, vc_cbhg_front's tiling restated, the
exact cases of tests/chain_cases.py exactly representable and able to see every layout, and every real-valued case's
derived bound below the flat tolerance the block tests allow."""
import numpy as np
import pytest
import torch

import chain_cases as Cs
import chain_ref as R

GATE_ERR = 4 * Cs.GATE_MAX


# ------------------------------------------------------------------------------------------ the reference itself

def _oracle_weights(p, n_hw):
    """chain_ref's matrices as the variable dictionary oracle/model_oracle.py reads (TF layouts; batch norm with mean 0 and
    variance 1 - eps, so that gamma is the folded scale and beta the folded shift)."""
    from oracle import model_oracle as mo
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    w = {'e/prenet/dense1/kernel': t(p['W1'].T), 'e/prenet/dense1/bias': t(p['b1']),
         'e/prenet/dense2/kernel': t(p['W2'].T), 'e/prenet/dense2/bias': t(p['b2'])}

    def conv(name, W, k, cin):
        w[name + '/conv1d/kernel'] = t(np.asarray(W).reshape(W.shape[0], k, cin).transpose(1, 2, 0))

    def norm(name, scale, shift):
        n = len(scale)
        w[name + '/gamma'], w[name + '/beta'] = t(scale), t(shift)
        w[name + '/moving_mean'], w[name + '/moving_variance'] = t(np.zeros(n)), t(np.full(n, 1.0 - mo.BN_EPS))
    for k in range(1, R.BANKS + 1):
        conv('e/CBHG/conv1d_banks/' + ('conv1d' if k == 1 else 'num_%d/conv1d' % k), p['bank'][k - 1], k, R.WIDTH)
    norm('e/CBHG/conv1d_banks/bn', p['bs'], p['bb'])
    conv('e/CBHG/conv1d_1', p['P1'], 3, R.BANKS * R.FILTERS)
    norm('e/CBHG/conv1d_1', p['p1s'], p['p1b'])
    conv('e/CBHG/conv1d_2', p['P2'], 3, R.WIDTH)
    norm('e/CBHG/conv1d_2', p['p2s'], p['p2b'])
    hr, tr = R.pair_rows(R.WIDTH)
    for i, (Wp, bp) in enumerate(p['hw']):
        s = 'e/CBHG/highwaynet_%d/' % i
        w[s + 'dense1/kernel'], w[s + 'dense1/bias'] = t(Wp[hr].T), t(bp[hr])
        w[s + 'dense2/kernel'], w[s + 'dense2/bias'] = t(Wp[tr].T), t(bp[tr])
    for d in ('fw', 'bw'):                                # the recurrence behind the tap is not under test: zeros
        s = 'e/CBHG/gru/bidirectional_rnn/%s/gru_cell/' % d
        w[s + 'gates/kernel'], w[s + 'gates/bias'] = t(np.zeros((2 * R.GRU, 2 * R.GRU))), t(np.zeros(2 * R.GRU))
        w[s + 'candidate/kernel'], w[s + 'candidate/bias'] = t(np.zeros((2 * R.GRU, R.GRU))), t(np.zeros(R.GRU))
    return w


@pytest.mark.parametrize('n_hw', [0, 2])
def test_reference_is_the_oracle_in_float64(n_hw):
    """prenet, cbhg (up to the tap behind the highway layers) and highwaynet of oracle/model_oracle.py against chain_ref
    with the roundings left out, 3 windows of 9 frames: float64 rounding apart."""
    from oracle import model_oracle as mo
    p = Cs.front_weights('real', n_hw)
    n, T = 3, 9
    X = Cs.front_input('real', n, T, 0)
    w = _oracle_weights(p, n_hw)
    x = torch.from_numpy(X).reshape(n, T, R.FEAT)
    pre = mo.prenet(x, w, 'e/prenet')
    taps = {}
    mo.cbhg(pre, w, 'e/CBHG', R.BANKS, n_hw, taps=taps)
    mine = {}
    xproj = R.front(X, p, T, taps=mine, rounding=False)
    for name, theirs in (('prenet', pre), ('bank', taps['banks']), ('conv1d_1', taps['proj1']), ('highway', taps['highway'])):
        a, b = mine[name].v, theirs.numpy().reshape(n * T, -1)
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), name
    assert np.abs(xproj.v - (mine['highway'].v @ p['Wx'].T + p['bx'])).max() <= 1e-12
    assert np.abs(R.pool_same(mine['bank'], T).v - mo.max_pool_2_same(taps['banks']).numpy().reshape(n * T, -1)).max() == 0.0
    # the highway layer and chain alone, 128 units
    layers, tail = Cs.highway_weights(128, 'real')
    Xh = Cs.highway_input(128, 'real', 33)
    Y, P = R.highway_chain(Xh, layers[:3], tail, rounding=False)
    y = torch.from_numpy(Xh)[None]
    hr, tr = R.pair_rows(128)
    for i, (Wp, bp) in enumerate(layers[:3]):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        hw = {'h/dense1/kernel': t(Wp[hr].T), 'h/dense1/bias': t(bp[hr]), 'h/dense2/kernel': t(Wp[tr].T), 'h/dense2/bias': t(bp[tr])}
        y = mo.highwaynet(y, hw, 'h')
    assert np.abs(Y.v - y[0].numpy()).max() <= 1e-12
    assert np.abs(P.v - (Y.v @ tail[0].T + tail[1])).max() <= 1e-12


def test_bf16_rounding_is_torchs_ties_included():
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.uniform(-6, 6, 20000), [Cs.TIE_DOWN, Cs.TIE_UP, -Cs.TIE_DOWN, -Cs.TIE_UP],
                        [0.0, -0.0, 1.0, 2.0 ** -126, 2.0 ** -133, 3.3895314e38, np.inf, -np.inf]]).astype(np.float32)
    base = R.from_bf16_bits(rng.randint(0, 0x7f80, 4000).astype(np.uint16))          # every tie: a bf16 number plus half an ulp
    ties = (base.view(np.uint32) | np.uint32(0x8000)).view(np.float32)
    x = np.concatenate([x, ties, -ties])
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.to_bf16_bits(x), want)
    assert np.array_equal(R.to_bf16(x), torch.from_numpy(x).bfloat16().double().numpy())
    assert R.to_bf16(Cs.TIE_DOWN) == 1.0 and R.to_bf16(Cs.TIE_UP) == 2.0          # one tie rounds down, one up
    assert np.isnan(R.to_bf16(np.float32('nan')))


# ------------------------------------------------------------------------------------------ layouts

def test_chained_kmap_is_what_the_register_hand_off_holds():
    """A result tile leaves v_mfma_f32_32x32x16 with register quad q of the lane half h holding channels 32 tile + 8 q + 4 h
    .. + 3; chain() of vc_cbhg_small.hip hands quads 2 (s & 1) and 2 (s & 1) + 1 of tile s >> 1 to k-step s as elements 0..3 and
    4..7.  The chained kmap is that, and a permutation of the K slots; the plain one is the identity."""
    for nks in (3, 5, 16, 32):
        slots = np.arange(16 * nks)
        s, h, e = slots >> 4, (slots >> 3) & 1, slots & 7
        quad = 2 * (s & 1) + (e >> 2)
        held = 32 * (s >> 1) + 8 * quad + 4 * h + (e & 3)
        assert np.array_equal(R.kmap(slots, 1), held)
        assert np.array_equal(np.sort(held), slots) if nks % 2 == 0 else set(held) >= set(range(16 * (nks - 1)))
        assert np.array_equal(R.kmap(slots, 0), slots)
    assert not np.array_equal(R.kmap(np.arange(80), 1), np.arange(80))


@pytest.mark.parametrize('rows,K,chained', [(40, 80, 1), (33, 17, 0), (128, 240, 0), (240, 40, 1), (1, 1, 0)])
def test_mfma_pack_formula_places_every_element_once(rows, K, chained):
    W = np.arange(1, rows * (K + 3) + 1, dtype=np.float64).reshape(rows, K + 3)          # ldw > K: the padding must not appear
    pk = R.mfma_pack(W, rows, K, chained)
    ntiles, nks = (rows + 31) // 32, (K + 15) // 16
    assert pk.shape == (ntiles * nks * 512,)
    assert np.array_equal(np.sort(pk[pk != 0]), np.sort(W[:, :K].reshape(-1)))
    f = pk.reshape(ntiles, nks, 64, 8)
    for tl, s, lane, e in ((0, 0, 0, 0), (ntiles - 1, nks - 1, 63, 7), (0, nks - 1, 37, 5)):
        row, col = 32 * tl + (lane & 31), int(R.kmap(16 * s + 8 * (lane >> 5) + e, chained))
        assert f[tl, s, lane, e] == (W[row, col] if row < rows and col < K else 0)


def test_highway_pack_formula():
    for H, n in ((128, 64), (256, 512)):
        Bt = np.arange(n * H, dtype=np.float64).reshape(n, H)
        pk = R.highway_pack(Bt, H).reshape(n // 64, H // 16, 2, 64, 8)
        assert np.array_equal(np.sort(pk.reshape(-1)), Bt.reshape(-1))
        for w, s, c, lane, j in ((0, 0, 0, 0, 0), (n // 64 - 1, H // 16 - 1, 1, 63, 7), (0, 3, 1, 40, 2)):
            assert pk[w, s, c, lane, j] == Bt[64 * w + 32 * c + (lane & 31), 16 * s + 8 * (lane >> 5) + j]


def test_proj1_reorder_and_coefficient_slots_are_the_host_codes():
    """modules._cbhg_front.build() restated: conv1d_1's TF kernel [3, 768, 40] goes through
    reshape(3, K, 4, 2, 16, Cw).permute(5, 1, 2, 0, 3, 4).reshape(Cw, 3 * 128 * K), and the coefficient vectors go to the
    offsets listed there."""
    K_, Cw = R.BANKS, R.WIDTH
    k1 = torch.arange(3 * 128 * K_ * Cw, dtype=torch.float64).reshape(3, 128 * K_, Cw)
    host = k1.reshape(3, K_, 4, 2, 16, Cw).permute(5, 1, 2, 0, 3, 4).reshape(Cw, 3 * 128 * K_).numpy()
    P1 = k1.numpy().transpose(2, 0, 1).reshape(Cw, 3 * 128 * K_)                      # [out, tap * 768 + channel]
    assert np.array_equal(R.proj1_reorder(P1), host)
    k, w, tap, s, j = 4, 2, 1, 1, 5                                                   # include/vc_hip.h's sentence, one element
    assert host[7, ((((k - 1) * 4 + w) * 3 + tap) * 2 + s) * 16 + j] == k1[tap, (k - 1) * 128 + 32 * w + 16 * s + j, 7]
    host_offsets = ((0, 'b1'), (96, 'b2'), (160, 'bs'), (1184, 'bb'), (2208, 'p1s'), (2272, 'p1b'), (2336, 'p2s'), (2400, 'p2b'), (2464, 'bx'))
    assert tuple((off, name) for name, off, _ in R.COEF_SLOTS) == host_offsets
    ends = [off + size for _, off, size in R.COEF_SLOTS]
    assert [off for _, off, _ in R.COEF_SLOTS][1:] + [R.COEF_HW] == ends                # slots tile [0, 2720) without a gap
    assert R.COEF_HW + R.COEF_HW_STRIDE * R.MAX_HIGHWAY == R.COEF_FLOATS == 3232
    p = Cs.front_weights('exact', 4)
    co = R.coef_table(p)
    assert np.array_equal(co[2272:2272 + 40], p['p1b'].astype(np.float32)) and not co[2272 + 40:2336].any()
    assert np.array_equal(co[2720 + 128 * 3:2720 + 128 * 4], p['hw'][3][1].astype(np.float32))


def test_listed_window_lengths_sit_on_the_tile_seams():
    """vc_cbhg_front restated: a block of 32 mi rows stores at most 32 mi - 10 frames (54 / 118); a window of T frames takes
    ceil(T / that) tiles of TF = ceil(T / tiles) frames.  The lists hold, per tile height: the smallest window, a full
    tile, one frame more (two tiles), and (mi = 2) two full tiles; then one frame more: three tiles, the last one short."""
    for mi, full in ((2, 54), (4, 118)):
        assert 32 * mi - (2 + (R.BANKS - 1) // 2) - 6 == full
        for T in Cs.FRONT_T[mi]:
            tiles, TF = R.front_tiles(T, mi)
            assert (tiles, TF, T - (tiles - 1) * TF) == Cs.FRONT_SEAMS[(mi, T)]
            assert TF <= full and (tiles - 1) * TF < T <= tiles * TF
        assert set(Cs.FRONT_T[mi]) >= {8, full, full + 1, 2 * full + 1}
        assert R.front_tiles(full, mi)[0] == 1 and R.front_tiles(full + 1, mi)[0] == 2 and R.front_tiles(2 * full + 1, mi)[0] == 3
        tiles, TF = R.front_tiles(2 * full + 1, mi)
        assert tiles * TF > 2 * full + 1 or mi == 4          # a short last tile (mi = 4: 3 x 79 = 237 exactly; 119 = 60 + 59 is short)
    assert R.front_tiles(119, 4) == (2, 60) and R.front_tiles(109, 2) == (3, 37)
    assert 108 in Cs.FRONT_T[2]


# ------------------------------------------------------------------------------------------ exact cases

@pytest.mark.parametrize('shape', Cs.PRENET_SHAPES)
def test_prenet_exact_cases_are_exactly_representable(shape):
    for inp, wk, xf in Cs.PRENET_EXACT:
        W1, b1, W2, b2 = Cs.prenet_weights(shape, wk)
        for M in Cs.PRENET_M:
            trace = []
            R.prenet(Cs.prenet_input(shape, inp, M), W1, b1, W2, b2, xf, trace)
            assert R.exactness(trace) is None, (inp, M, R.exactness(trace))
    # one-hot rows show every dense1 weight singly: the dense1 output of row m is relu(W1[:, m] + b1)
    W1, b1, W2, b2 = Cs.prenet_weights(shape, 'onehot')
    X = Cs.prenet_input(shape, 'onehot', 257)
    assert np.array_equal(np.maximum(X @ W1.T + b1, 0)[:shape[0]], np.maximum(W1.T + b1, 0)) and len(np.unique(W1)) == 15
    assert (np.abs(W2).sum(0) > 0).all()


@pytest.mark.parametrize('H', Cs.HIGHWAY_H)
def test_highway_exact_cases_are_exactly_representable(H):
    for L in Cs.HIGHWAY_LAYERS:
        for M in sorted(set(Cs.HIGHWAY_M) | {H}):
            X, Y, P, trace = Cs.highway_case(H, 'exact', L, M)
            assert R.exactness(trace) is None, (L, M, R.exactness(trace))
            assert np.array_equal(P.v.astype(np.float32).astype(np.float64), P.v)
    # identity rows: output [m, u] of the first layer is gate(W2[u, m]) applied to relu(W1[u, m] + b1[u]) and the identity
    layers, _ = Cs.highway_weights(H, 'exact')
    Wp, bp = layers[0]
    hr, tr = R.pair_rows(H)
    _, Y, _, _ = Cs.highway_case(H, 'exact', 1, H)
    h, t = np.maximum(Wp[hr].T + bp[hr], 0), {0.0: 0.5, 2048.0: 1.0, -2048.0: 0.0}
    tv = np.vectorize(t.get)(Wp[tr].T)
    assert np.array_equal(Y.v, tv * (h - np.eye(H)) + np.eye(H))
    assert set(np.unique(Wp[tr])) == {0.0, 2048.0, -2048.0} and not bp[tr].any()


@pytest.mark.parametrize('mi', [2, 4])
def test_front_exact_cases_are_exactly_representable(mi):
    for L, n, T, xf in Cs.front_exact_list(mi):
        X, xproj, trace = Cs.front_case('exact', L, n, T, xf)
        assert R.exactness(trace) is None, (L, n, T, xf, R.exactness(trace))
        assert np.array_equal(xproj.v.astype(np.float32).astype(np.float64), xproj.v)
    p = Cs.front_weights('exact', 4)
    assert (p['bb'] != 0).all(), 'a zero bank shift hides a frame outside the window that was not zeroed'
    assert all((np.abs(p['P1'][:, 16 * g:16 * g + 16]).sum() > 0) for g in range(3 * R.BANKS * R.FILTERS // 16))
    for k, b in enumerate(p['bank'], 1):                 # every width, every tap, every 32-channel slice
        assert (np.abs(b).reshape(4, 32, k, R.WIDTH).sum(axis=(1, 3)) > 0).all(), k
    assert {0.0, 2048.0, -2048.0} == set(np.unique(p['hw'][0][1][R.pair_rows(R.WIDTH)[1]]))


# ------------------------------------------------------------------------------------------ the exact cases see the layouts

def _front_out(p, L=0, n=3, T=9, xf=0):
    return R.front(Cs.front_input('exact', n, T, xf), p, T, bool(xf)).v


def _p1_cols(k1=slice(None), w=slice(None), tap=slice(None), s=slice(None)):
    idx = np.arange(3 * R.BANKS * R.FILTERS).reshape(3, R.BANKS, 4, 2, 16)              # [tap, width, slice, half, j]
    return idx[tap, k1, w, s].reshape(-1)


def _swapped_cols(W, a, b):
    W = W.copy()
    W[:, np.concatenate([a, b])] = W[:, np.concatenate([b, a])]
    return W


def _front_mutations():
    """name -> function(p) returning the weights a kernel that mixes up the named layout would effectively use."""
    def p1(a, b):
        return lambda p: dict(p, P1=_swapped_cols(p['P1'], _p1_cols(**a), _p1_cols(**b)))
    m = {'proj1: widths 1 and 2': p1(dict(k1=0), dict(k1=1)), 'proj1: widths 5 and 6': p1(dict(k1=4), dict(k1=5)),
         'proj1: slices 0 and 1': p1(dict(w=0), dict(w=1)), 'proj1: slices 2 and 3': p1(dict(w=2), dict(w=3)),
         'proj1: taps 0 and 1': p1(dict(tap=0), dict(tap=1)), 'proj1: taps 1 and 2': p1(dict(tap=1), dict(tap=2)),
         'proj1: halves': p1(dict(s=0), dict(s=1))}

    def bank_ranges(p):                                   # width 5 read where width 6 lies and the other way round
        b = list(p['bank'])
        b[4], b[5] = p['bank'][5][:, :200], np.concatenate([p['bank'][4], np.zeros((R.FILTERS, 40))], axis=1)
        return dict(p, bank=b)

    def bank_taps(p):
        b = list(p['bank'])
        b[5] = _swapped_cols(b[5], np.arange(0, 40), np.arange(40, 80))
        return dict(p, bank=b)

    def bank_last_taps(p):
        b = list(p['bank'])
        b[5] = _swapped_cols(b[5], np.arange(160, 200), np.arange(200, 240))
        return dict(p, bank=b)
    m.update({'bank: ranges of widths 5 and 6': bank_ranges, 'bank: taps 0 and 1 of k = 6': bank_taps, 'bank: taps 4 and 5 of k = 6': bank_last_taps})
    m['proj2: taps 0 and 2'] = lambda p: dict(p, P2=_swapped_cols(p['P2'], np.arange(0, 40), np.arange(80, 120)))

    def gru_blocks(p):
        W, b = p['Wx'].copy(), p['bx'].copy()
        W[np.r_[0:80, 120:200]] = W[np.r_[120:200, 0:80]]
        return dict(p, Wx=W)
    m['gru: fw and bw gate row blocks'] = gru_blocks
    names = [n for n, _, _ in R.COEF_SLOTS]
    for i, name in enumerate(names):                      # a vector read from its right-hand neighbour's slot
        nb = names[(i + 1) % len(names)]

        def shifted(p, name=name, nb=nb):
            v = np.zeros(len(p[name]))
            k = min(len(v), len(p[nb]))
            v[:k] = np.asarray(p[nb])[:k]
            return dict(p, **{name: v})
        m['coef: %s from the slot of %s' % (name, nb)] = shifted
    for name in ('W2', 'Wx'):                            # a chained matrix packed plainly
        def plain(p, name=name):
            K = p[name].shape[1]
            held = R.kmap(np.arange(K), 1)               # slot i multiplies channel held[i] with the weight of column i
            W = np.zeros_like(p[name])
            W[:, held[held < K]] = p[name][:, np.arange(K)[held < K]]
            return dict(p, **{name: W})
        m['kmap: %s plain instead of chained' % name] = plain
    return m


@pytest.mark.parametrize('name', sorted(_front_mutations()))
def test_front_exact_cases_see_the_layout(name):
    p = Cs.front_weights('exact', 0)
    q = _front_mutations()[name](p)
    assert any(not np.array_equal(_front_out(p, xf=xf), _front_out(q, xf=xf)) for xf in (0, 1)), name


def test_front_exact_cases_see_the_highway_layouts():
    p = Cs.front_weights('exact', 4)
    base = _front_out(p)
    hr, tr = R.pair_rows(R.WIDTH)
    for l in range(4):
        Wp, bp = p['hw'][l]
        swapped_w, swapped_b, nxt = Wp.copy(), bp.copy(), p['hw'][(l + 1) % 4][1]
        swapped_w[np.r_[0:32, 32:64]] = Wp[np.r_[32:64, 0:32]]                       # dense1 / dense2 rows of pair block 0
        swapped_b[np.r_[0:32, 32:64]] = bp[np.r_[32:64, 0:32]]                       # bH / bT offsets exchanged
        for what, layer in (('weights', (swapped_w, bp)), ('biases', (Wp, swapped_b)), ('next layer biases', (Wp, nxt))):
            hw = list(p['hw'])
            hw[l] = layer
            assert not np.array_equal(base, _front_out(dict(p, hw=hw))), (l, what)


@pytest.mark.parametrize('H', Cs.HIGHWAY_H)
def test_highway_exact_cases_see_the_layouts(H):
    layers, tail = Cs.highway_weights(H, 'exact')
    for M in (H, 300):
        X = Cs.highway_input(H, 'exact', M)
        Y0, P0 = R.highway_chain(X, layers, tail)
        for l in (0, 1, 7):
            Wp, bp = layers[l]
            for a, b in ((np.arange(0, 32), np.arange(32, 64)), (np.arange(0, 64), np.arange(64, 128))):   # dense1 / dense2; two waves
                W2, b2 = Wp.copy(), bp.copy()
                W2[np.concatenate([a, b])], b2[np.concatenate([a, b])] = Wp[np.concatenate([b, a])], bp[np.concatenate([b, a])]
                ls = list(layers)
                ls[l] = (W2, b2)
                Y, P = R.highway_chain(X, ls, tail)
                assert not np.array_equal(Y.v, Y0.v) and not np.array_equal(P.v, P0.v), (M, l)
            ls = list(layers)
            ls[l] = (_swapped_cols(Wp, np.arange(0, 8), np.arange(8, 16)), bp)                              # two K slots of 8
            assert not np.array_equal(R.highway_chain(X, ls, tail)[0].v, Y0.v), (M, l)
        # the last layer left out (the final tile taken from the other buffer), and two tail column groups exchanged
        assert not np.array_equal(R.highway_chain(X, layers[:7], tail)[0].v, Y0.v)
        PW = tail[0].copy()
        PW[np.r_[0:64, 64:128]] = tail[0][np.r_[64:128, 0:64]]
        assert not np.array_equal(R.highway_chain(X, layers, (PW, tail[1]))[1].v, P0.v)
        # the stored tile without its swizzle: 16-byte slot s of row r read at s ^ (r & 15)
        r, s = np.meshgrid(np.arange(M), np.arange(H // 8), indexing='ij')
        unsw = Y0.v.reshape(M, H // 8, 8)[r, s ^ (r & 15)].reshape(M, H)
        assert not np.array_equal(unsw, Y0.v)


@pytest.mark.parametrize('shape', Cs.PRENET_SHAPES)
def test_prenet_exact_cases_see_the_layouts(shape):
    cin, u1, u2 = shape
    for inp, wk, xf in Cs.PRENET_EXACT:
        W1, b1, W2, b2 = Cs.prenet_weights(shape, wk)
        X = Cs.prenet_input(shape, inp, 257)
        y0 = R.prenet(X, W1, b1, W2, b2, xf).v
        src = R.kmap(np.arange(u1), 1)
        variants = {'dense2 plain instead of chained': (W1, b1, W2[:, src], b2),
                    'dense2 bias of the neighbouring tile': (W1, b1, W2, b2.reshape(-1, 32)[np.arange(u2 // 32) ^ 1].reshape(-1)),
                    'dense1 bias of the neighbouring tile': (W1, b1.reshape(-1, 32)[np.arange(u1 // 32) ^ 1].reshape(-1), W2, b2),
                    'two k-steps of dense1': (_swapped_cols(W1, np.arange(0, 16), np.arange(16, 32)), b1, W2, b2),
                    'two tiles of dense1': (W1[np.r_[32:64, 0:32, 64:u1]], b1, W2, b2)}
        for name, (a, b, c, d) in variants.items():
            if inp == 'ints' and name == 'two k-steps of dense1':
                continue                                  # rows of ones weigh every K slot alike only by chance; the one-hot rows decide
            assert not np.array_equal(R.prenet(X, a, b, c, d, xf).v, y0), (inp, name)
    # truncating instead of rounding the float32 features moves the ties case
    W1, b1, W2, b2 = Cs.prenet_weights(shape, 'onehot')
    X = Cs.prenet_input(shape, 'ties', 257)
    trunc = (X.astype(np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)
    assert not np.array_equal(R.prenet(trunc, W1, b1, W2, b2, False).v, R.prenet(X, W1, b1, W2, b2, True).v)


# ------------------------------------------------------------------------------------------ real-valued cases

def _below_flat(t, what):
    scale = max(1.0, float(np.abs(t.v).max()))
    assert float(t.e.max()) <= Cs.FLAT_BF16 * scale, (what, float(t.e.max()), scale)
    assert float(t.e.max()) > 0.0


def test_real_valued_bounds_stay_below_the_flat_tolerance():
    """Nothing is loosened: on every real-valued device input the derived bound, element by element, is below
    3e-2 max(1, max |reference|), which is all tests/test_blocks_gpu.py asks of these kernels."""
    assert GATE_ERR <= 2e-5
    for shape in Cs.PRENET_SHAPES:
        W1, b1, W2, b2 = Cs.prenet_weights(shape, 'real')
        for xf in (0, 1):
            _below_flat(R.prenet(Cs.prenet_input(shape, 'real', 257), W1, b1, W2, b2, xf), ('prenet', shape))
    for H in Cs.HIGHWAY_H:
        for L in Cs.HIGHWAY_LAYERS:
            for M in Cs.HIGHWAY_M:
                _, Y, P, _ = Cs.highway_case(H, 'real', L, M, GATE_ERR)
                if L:
                    _below_flat(Y, ('highway', H, L, M))
                _below_flat(P, ('highway tail', H, L, M))
    for mi in (2, 4):
        for L, n, T, xf in Cs.front_real_list(mi):
            _below_flat(Cs.front_case('real', L, n, T, xf, GATE_ERR)[1], ('front', L, n, T, xf))


def _without_one_weight(W):
    W = W.copy()
    nz = np.argwhere(W != 0)
    W[tuple(nz[len(nz) // 2])] = 0.0
    return W


def test_what_the_real_valued_bounds_can_and_cannot_see():
    """A worst-case bound through up to ten rounding points is wide: losing ONE weight of the last linear layer in front of an
    output moves it by more than the bound (prenet: both layers), losing one weight of an early layer of the front does
    not (0.2 .. 0.8 of the bound).  That is why layouts and edges are the exact cases' job; the real-valued cases hold the
    arithmetic (accumulation, gate, rounding points) to what the number formats allow."""
    for shape in Cs.PRENET_SHAPES:
        W1, b1, W2, b2 = Cs.prenet_weights(shape, 'real')
        X = Cs.prenet_input(shape, 'real', 257)
        y = R.prenet(X, W1, b1, W2, b2)
        assert (np.abs(R.prenet(X, _without_one_weight(W1), b1, W2, b2).v - y.v) > y.e).any()
        assert (np.abs(R.prenet(X, W1, b1, _without_one_weight(W2), b2).v - y.v) > y.e).any()
    p = Cs.front_weights('real', 1)
    X, ref, _ = Cs.front_case('real', 1, 3, 55, 0, GATE_ERR)
    assert (np.abs(R.front(X, dict(p, Wx=_without_one_weight(p['Wx'])), 55).v - ref.v) > ref.e).any()
    assert not (np.abs(R.front(X, dict(p, W1=_without_one_weight(p['W1'])), 55).v - ref.v) > ref.e).any()
    for H in Cs.HIGHWAY_H:
        layers, tail = Cs.highway_weights(H, 'real')
        X, Y, P, _ = Cs.highway_case(H, 'real', 8, 300, GATE_ERR)
        Wp, bp = layers[7]
        W = Wp.copy()
        hr = R.pair_rows(H)[0]
        W[hr] = _without_one_weight(Wp[hr])
        Y2, _ = R.highway_chain(X, layers[:7] + [(W, bp)], tail, GATE_ERR)
        assert (np.abs(Y2.v - Y.v) > Y.e).any()
