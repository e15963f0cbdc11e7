"""The speaker launches alone, through the C ABI with raw pointers: vc_spk_features_f32, vc_gmm_prepare_f32,
vc_gmm_loglik_f32, vc_gmm_score_f32, vc_gmm_accumulate_f32 (with its reduction launch), vc_gmm_update_f32 and the four
queries of csrc/vc_gmm.hip -- against tests/speaker_ref.py on the cases of tests/speaker_kernels_cases.py
(tests/test_speaker_kernels_cpu.py proves those usable and pins the bounds).

The memory contract of every test: it starts with poison_gpu_state(); every output and the workspace lie between two
256-byte bands of sentinels that are checked after each call; the workspace is exactly vc_gmm_workspace_bytes long and
starts as 0xA5 bytes; outputs start as the sentinel and none may remain where the header says every element is written;
inputs hold NaN (0x7fffffff, set mask bytes) wherever the header says nothing is read -- features, cepstra, ll and mask
behind len[b]; every launch runs twice into fresh sentinels and the raw bits agree; for the three score launches row b of
the dirty ragged batch equals, bit for bit, utterance b alone in tight clean buffers.  Exact cases are compared bit for
bit; a real-valued one prints a line starting with MEASURED with its error, bound and ratio
(profiles/speaker_kernels/README.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import speaker_kernels_cases as Cs
import speaker_ref as sr
from conftest import poison_gpu_state

pytestmark = pytest.mark.gpu

VC_ERR_INVALID, VC_ERR_WORKSPACE, VC_ERR_UNSUPPORTED = 1, 3, 4
CAN32, CAN8, CAN64 = 0x7FA5A5A5, 0xA5, 0x7FF5A5A5A5A5A5A5      # NaNs with a payload no arithmetic produces
BAND = 256                                                     # sentinel bytes on either side
IFILL = Cs.IFILL


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


def _refused(rc, code, text=''):
    msg = _lib().vc_last_error().decode()
    assert rc == code and text in msg, (rc, code, msg)


class Buf:
    """n elements of float32 / int32 ('f', 'i'), float64 ('d') or bytes ('b') between two bands of sentinels."""
    KINDS = {'f': (torch.int32, CAN32), 'i': (torch.int32, CAN32), 'd': (torch.int64, CAN64), 'b': (torch.uint8, CAN8)}

    def __init__(self, n, kind='f'):
        self.n, self.kind = int(n), kind
        self.idt, self.can = self.KINDS[kind]
        self.raw = torch.full((1,), self.can, dtype=self.idt, device='cuda')
        self.pad = BAND // self.raw.element_size()
        self.raw = torch.full((self.n + 2 * self.pad,), self.can, dtype=self.idt, device='cuda')

    def ptr(self, off=0):
        return C.c_void_p(self.raw.data_ptr() + self.pad * self.raw.element_size() + off)

    def bands_ok(self):
        torch.cuda.synchronize()
        return bool((self.raw[:self.pad] == self.can).all()) and bool((self.raw[self.pad + self.n:] == self.can).all())

    def bits(self, shape=None, written=True):
        """The body's bits on the host; the bands must be intact and, by default, no sentinel left inside."""
        assert self.bands_ok(), 'wrote outside the buffer'
        body = self.raw[self.pad:self.pad + self.n].cpu().numpy().copy()
        if written and self.kind != 'b':
            assert not (body == self.can).any(), '%d elements were never written' % int((body == self.can).sum())
        return body if shape is None else body.reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == self.can).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def i32(v):
    return dev(np.asarray(v, dtype=np.int64).astype(np.int32))


def f32(bits):
    return bits.view(np.float32)


def f64(bits):
    return bits.view(np.float64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(autouse=True)
def _own_line():
    print()                                                              # (-s: the MEASURED lines start their own line)
    yield


def twice(run, what):
    """run() -> dict of host bit arrays: two launches into fresh sentinels, identical bits; the first one's."""
    a, b = run(), run()
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), '%s: two launches differ in %s' % (what, k)
    return a


def measured(what, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
    print('MEASURED %s err=%.3e bound=%.3e err/bound=%.3f' % (what, err, bound, ratio))
    return ratio


# ================================================================================================ the launches
def run_features(cep, lens, mask, deltas, cmn):
    B, F, n_coef = cep.shape
    D = n_coef * (1 + deltas)
    d_cep, d_len, d_mask = dev(cep), i32(lens), None if mask is None else dev(mask)
    out = Buf(B * F * D)
    _ok(_lib().vc_spk_features_f32(ptr(d_cep), ptr(d_len), ptr(d_mask), B, F, n_coef, deltas, cmn, out.ptr(), _st()))
    return dict(feat=out.bits((B, F, D)))


def run_prepare(w, mu, var):
    """The table between its bands (kept on the device for the launches that read it) and its bits."""
    lib = _lib()
    S, M, D = mu.shape
    n = lib.vc_gmm_table_floats(S, M, D)
    assert n == Cs.table_floats(S, M, D)
    d_w, d_mu, d_var = dev(w), dev(mu), dev(var)
    tab = Buf(n)
    _ok(lib.vc_gmm_prepare_f32(ptr(d_w), ptr(d_mu), ptr(d_var), S, M, D, tab.ptr(), _st()))
    return tab, tab.bits()


def run_loglik(x, lens, tab, S, M, model_a, model_b=None):
    B, F, D = x.shape
    d_x, d_len, d_a = dev(x), i32(lens), i32(model_a)
    d_b = None if model_b is None else i32(model_b)
    ll_a = Buf(B * F)
    ll_b = None if model_b is None else Buf(B * F)
    _ok(_lib().vc_gmm_loglik_f32(ptr(d_x), ptr(d_len), B, F, D, tab.ptr(), S, M, ptr(d_a), ll_a.ptr(), ptr(d_b),
                                 None if ll_b is None else ll_b.ptr(), _st()))
    assert tab.bands_ok()
    out = dict(ll_a=ll_a.bits((B, F)))
    if ll_b is not None:
        out['ll_b'] = ll_b.bits((B, F))
    return out


def run_score(a, b_, lens, mask):
    B, F = a.shape
    d_a, d_b, d_len, d_mask = dev(a), None if b_ is None else dev(b_), i32(lens), None if mask is None else dev(mask)
    n, v = Buf(B, 'i'), Buf(3 * B)
    _ok(_lib().vc_gmm_score_f32(ptr(d_a), ptr(d_b), ptr(d_len), ptr(d_mask), B, F, n.ptr(), v.ptr(), _st()))
    return dict(n=n.bits(), values=v.bits((B, 3)))


def run_accumulate(x, ll, lens, mask, groups, tab, S, M, model, G, null_ws=False):
    """ll: float32 [B, F] on the host (NaN behind the lengths).  The workspace is exactly the queried size, 0xA5 bytes."""
    lib = _lib()
    B, F, D = x.shape
    need = lib.vc_gmm_workspace_bytes(G, M, D)
    assert need == Cs.workspace_bytes(G, M, D)
    d_x, d_ll, d_len, d_g = dev(x), dev(ll), i32(lens), i32(groups)
    d_mask = None if mask is None else dev(mask)
    ws = Buf(need, 'b')
    N, S1, S2, L = Buf(G * M, 'd'), Buf(G * M * D, 'd'), Buf(G * M * D, 'd'), Buf(G, 'd')
    assert not (null_ws and need)
    _ok(lib.vc_gmm_accumulate_f32(ptr(d_x), ptr(d_ll), ptr(d_len), ptr(d_mask), ptr(d_g), B, F, D, tab.ptr(), S, M, model, G, N.ptr(),
                                  S1.ptr(), S2.ptr(), L.ptr(), None if null_ws else ws.ptr(), 0 if null_ws else need, _st()))
    assert ws.bands_ok() and tab.bands_ok(), 'wrote outside the workspace'
    return dict(N=N.bits((G, M)), S1=S1.bits((G, M, D)), S2=S2.bits((G, M, D)), L=L.bits())


def run_update(mode, N, S1, S2, mu_in, var_in, floor, min_count, relevance, nulls=False):
    N, S1 = np.asarray(N, np.float64), np.asarray(S1, np.float64)
    G, M = N.shape
    D = S1.shape[2]
    d_N, d_S1, d_mu = dev(N), dev(S1), dev(mu_in)
    d_S2 = None if (mode == 1 and nulls) else dev(np.asarray(S2, np.float64))
    d_var = None if (mode == 1 and nulls) else dev(var_in)
    d_fl = None if (mode == 1 and nulls) else dev(floor)
    mu = Buf(G * M * D)
    w, var = (None, None) if (mode == 1 and nulls) else (Buf(M), Buf(M * D))
    _ok(_lib().vc_gmm_update_f32(mode, ptr(d_N), ptr(d_S1), ptr(d_S2), G, M, D, ptr(d_mu), ptr(d_var), ptr(d_fl), min_count, relevance,
                                 None if w is None else w.ptr(), mu.ptr(), None if var is None else var.ptr(), _st()))
    out = dict(mu=mu.bits((G, M, D)))
    if mode == 0:
        out.update(w=w.bits(), var=var.bits((M, D)))
    elif w is not None:
        assert w.untouched() and var.untouched()                        # the MAP mode writes means only
    return out


def ulps(got, want):
    want = np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ================================================================================================ queries
def test_queries_equal_the_restated_geometry():
    lib = _lib()
    assert lib.vc_gmm_tile_frames() == Cs.TILE
    for G in (1, 2, 3, 4, 42, 43, 63, 64, 65, 127, 128, 129, 4095, 4096):
        assert lib.vc_gmm_partitions(G) == Cs.partitions(G), G
        for M, D in ((1, 1), (64, 5), (65, 48), (256, 64)):
            assert lib.vc_gmm_workspace_bytes(G, M, D) == Cs.workspace_bytes(G, M, D), (G, M, D)
    assert lib.vc_gmm_partitions(0) == 0 and lib.vc_gmm_partitions(4097) == 0 and lib.vc_gmm_partitions(-1) == 0
    assert lib.vc_gmm_workspace_bytes(1, 257, 1) == 0 and lib.vc_gmm_workspace_bytes(1, 1, 65) == 0 and lib.vc_gmm_workspace_bytes(0, 1, 1) == 0
    for S, M, D in Cs.PREP_SHAPES:
        assert lib.vc_gmm_table_floats(S, M, D) == Cs.table_floats(S, M, D)
    assert lib.vc_gmm_table_floats(4098, 1, 1) == 0 and lib.vc_gmm_table_floats(4097, 1, 1) == 4098 + 1


# ================================================================================================ features
def _feat_alone(cep_b, e, mask_b, deltas, cmn):
    """Utterance b alone in tight clean buffers: max_frames = len (one zero row when it has no frame)."""
    if e == 0:
        return run_features(np.zeros((1, 1, cep_b.shape[1]), np.float32), [0], None if mask_b is None else np.ones((1, 1), np.uint8), deltas, cmn)
    return run_features(cep_b[None, :e].copy(), [e], None if mask_b is None else (mask_b[None, :e] != 0).astype(np.uint8), deltas, cmn)


@pytest.mark.parametrize('deltas', [0, 1])
@pytest.mark.parametrize('n_coef', Cs.FEAT_COEF)
def test_features_ragged_dirty_batch(n_coef, deltas):
    """len -5 .. max_frames + 100 (the clamp, the four delta index clamps, zero rows from len on), NaN rows behind every
    length; D = 1 and D = 64.  Real-valued cepstra within 8 u A of float64; integer cepstra bit for bit the float32
    restatement; every row as the utterance alone; no mask as every byte set; no kept frame as cmn = 0."""
    poison_gpu_state()
    cep, mask = Cs.feat_batch(n_coef)
    res = twice(lambda: run_features(cep, Cs.FEAT_LENS, mask, deltas, 1), 'vc_spk_features_f32')
    got = f32(res['feat'])
    worst = (0.0, 0.0)
    for b, n in enumerate(Cs.FEAT_LENS):
        e = Cs.feat_eff(n)
        assert not res['feat'][b, e:].any(), (b, 'rows from len on are +0')
        alone = _feat_alone(cep[b], e, mask[b], deltas, 1)
        assert np.array_equal(alone['feat'][0, :e], res['feat'][b, :e]), (b, 'alone against the batch')
        if e:
            want = sr.features(Cs.clean(cep[b]), e, mask[b], bool(deltas), True)
            err, bound = float(np.abs(got[b] - want).max()), Cs.feat_bound(float(np.abs(cep[b, :e]).max()))
            worst = max(worst, (err / bound, err, bound))
            assert err <= bound, (b, n, err, bound)
    assert measured('vc_spk_features_f32 nc%d deltas%d' % (n_coef, deltas), worst[1], worst[2]) <= 1.0
    icep, imask = Cs.feat_batch(n_coef, integer=True)
    ires = twice(lambda: run_features(icep, Cs.FEAT_LENS, imask, deltas, 1), 'integer cepstra')
    every = run_features(icep, Cs.FEAT_LENS, None, deltas, 1)
    ones = run_features(icep, Cs.FEAT_LENS, np.ones_like(imask), deltas, 1)
    none = run_features(icep, Cs.FEAT_LENS, np.zeros_like(imask), deltas, 1)
    plain = run_features(icep, Cs.FEAT_LENS, imask, deltas, 0)
    assert np.array_equal(every['feat'], ones['feat']) and np.array_equal(none['feat'], plain['feat'])
    for b, n in enumerate(Cs.FEAT_LENS):
        for r, mk, cmn in ((ires, imask[b], True), (every, None, True), (plain, imask[b], False)):
            want = sr.features_f32(icep[b], n, mk, bool(deltas), cmn)
            assert np.array_equal(r['feat'][b], bits32(want)), (b, n, cmn, 'integer cepstra: bits of the float32 restatement')


def test_features_one_kept_frame_in_each_lane_is_the_mean():
    """One kept frame f, f mod 4 = 0 .. 3: the mean is that frame's feature (a float64 sum of one term over a count of
    one), its row comes out as zeros, every other row as one rounded difference: bits of the float32 restatement."""
    poison_gpu_state()
    rng = np.random.RandomState(8)
    F, n_coef = 20 + Cs.PAD, 5
    cep = np.full((len(Cs.ONE_KEPT), F, n_coef), np.nan, np.float32)
    cep[:, :20] = rng.randint(-8, 9, (len(Cs.ONE_KEPT), 20, n_coef))
    mask = np.zeros((len(Cs.ONE_KEPT), F), np.uint8)
    mask[:, 20:] = 0xA5
    for b, f in enumerate(Cs.ONE_KEPT):
        mask[b, f] = 1
    res = twice(lambda: run_features(cep, [20] * len(Cs.ONE_KEPT), mask, 1, 1), 'one kept frame')
    for b, f in enumerate(Cs.ONE_KEPT):
        assert not res['feat'][b, f].any() and res['feat'][b, :20].any()
        assert np.array_equal(res['feat'][b], bits32(sr.features_f32(cep[b], 20, mask[b], True, True))), f
    # two kept frames in lanes 3 and 0, in that order of frames: the sum is (lane 0) + (lane 3)
    mask[0, :20] = 0
    mask[0, [7, 16]] = 1
    res = run_features(cep, [20] * len(Cs.ONE_KEPT), mask, 1, 1)
    assert np.array_equal(res['feat'][0], bits32(sr.features_f32(cep[0], 20, mask[0], True, True)))


def test_features_mean_is_summed_in_the_documented_order():
    """Cepstra of +-2^e over sixty binades (deltas = 0, so a feature is its cepstrum): the float64 column sums are inexact
    and depend on their order -- lane r adds the kept frames r, r + 4, ... ascending, then ((0 + 1) + 2) + 3 --; the mean
    is rounded once and subtracted with one rounding: bits of the order-following restatement.  The last utterance makes the
    order of the four partial sums visible after the rounding to float32: 2^100, 1, -2^100, 1 in lanes 0 .. 3 sum to 1 as
    ((0 + 1) + 2) + 3 (the first 1 is absorbed, the second is not) and to 0 as (0 + 1) + (2 + 3)."""
    poison_gpu_state()
    rng = np.random.RandomState(21)
    lens, n_coef = [37, 5, 64, 3, 4], 7
    F = max(lens) + Cs.PAD
    cep = np.full((len(lens), F, n_coef), np.nan, np.float32)
    for b, n in enumerate(lens):
        cep[b, :n] = np.where(rng.rand(n, n_coef) < 0.5, -1.0, 1.0) * 2.0 ** rng.randint(-30, 31, (n, n_coef))
    mask = Cs.random_mask(rng, lens, F, 0.8)
    cep[4, :4] = np.array([2.0 ** 100, 1.0, -2.0 ** 100, 1.0], np.float32)[:, None]
    mask[4, :4] = 1
    assert sr.features_f32(cep[4], 4, mask[4], False, True)[1, 0] == 0.75                    # the mean is 1 / 4
    res = twice(lambda: run_features(cep, lens, mask, 0, 1), 'wide-range cepstra')
    for b, n in enumerate(lens):
        assert np.array_equal(res['feat'][b], bits32(sr.features_f32(cep[b], n, mask[b], False, True))), b


# ================================================================================================ prepare
@pytest.mark.parametrize('shape', Cs.PREP_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_prepare_table_values(shape):
    """Means are bit copies in [s][d][m]; 1 / var is float32(1.0 / float64(var)) exactly; c_m within half a float32 ulp plus
    the float64 term count; a weight of exactly 0 gives c_m = -inf.  Table sizes either side of 256 and 512 floats."""
    poison_gpu_state()
    S, M, D = shape
    zero = M // 2 if M > 1 else None
    w, mu, var = Cs.prep_model(S, M, D, zero)
    res = twice(lambda: dict(tab=run_prepare(w, mu, var)[1]), 'vc_gmm_prepare_f32')['tab']
    n_mu, n_iv = S * M * D, M * D
    assert np.array_equal(res[:n_mu].reshape(S, D, M), bits32(mu.transpose(0, 2, 1)))
    iv = (1.0 / var.astype(np.float64)).astype(np.float32)
    assert np.array_equal(res[n_mu:n_mu + n_iv].reshape(D, M), bits32(iv.T))
    c = f32(res[n_mu + n_iv:]).astype(np.float64)
    want, bound = Cs.c_reference(w, var)
    live = np.isfinite(want)
    assert live.sum() == M - (zero is not None) and np.isneginf(c[~live]).all() and not np.isnan(c).any()
    err = np.abs(c[live] - want[live])
    k = int(np.argmax(err / bound[live]))
    assert measured('vc_gmm_prepare_f32 c_m %dx%dx%d' % shape, float(err[k]), float(bound[live][k])) <= 1.0


# ================================================================================================ loglik
def _ll_check(c, res_bits, models, what):
    """Rows against float64 within sr.frame_bound; +0 from len on; returns (ratio, err, bound) of the worst frame."""
    got = f32(res_bits)
    worst = (0.0, 0.0, 0.0)
    for b, e in enumerate(c['eff']):
        assert not res_bits[b, e:].any(), (what, b, 'zeros from len on')
        if e:
            want, E = sr.loglik(c['x'][b, :e], c['w'], c['mu'][models[b]], c['var'])
            bound = sr.frame_bound(c['D'], c['M'], E)
            err = np.abs(got[b, :e] - want)
            assert np.isfinite(got[b, :e]).all() and (err <= bound).all(), (what, b, float((err / bound).max()))
            k = int(np.argmax(err / bound))
            worst = max(worst, (float(err[k] / bound[k]), float(err[k]), float(bound[k])))
    return worst


@pytest.mark.parametrize('D', Cs.LL_DS)
@pytest.mark.parametrize('M', Cs.LL_MS)
def test_loglik_component_seams(M, D):
    """Every `lane + 64 k < M` seam at D = 1, 63, 64; lengths 0 .. 70 in 70 frames (the eight-frame groups, a tile wholly or
    partly past len, n_out = 6 in the last tile); hard_case's narrow component and its frame 40 sigma out; model indices
    -3, 0, S - 1, S + 5; NaN features behind every length; every row as the utterance alone."""
    poison_gpu_state()
    c = Cs.ll_case(D, M, 2, 70)
    raw, eff = Cs.ll_model_index(2)
    tab, _ = run_prepare(c['w'], c['mu'], c['var'])
    res = twice(lambda: run_loglik(c['x'], c['lens'], tab, 2, M, raw, raw[::-1]), 'vc_gmm_loglik_f32')
    wa = _ll_check(c, res['ll_a'], eff, 'first model')
    wb = _ll_check(c, res['ll_b'], eff[::-1], 'second model')
    worst = max(wa, wb)
    assert measured('vc_gmm_loglik_f32 M%d D%d' % (M, D), worst[1], worst[2]) <= 1.0
    for b, e in enumerate(c['eff']):
        if e:
            alone = run_loglik(c['x'][b:b + 1, :e].copy(), [e], tab, 2, M, [eff[b]], [eff[::-1][b]])
            assert np.array_equal(alone['ll_a'][0], res['ll_a'][b, :e]) and np.array_equal(alone['ll_b'][0], res['ll_b'][b, :e]), b


@pytest.mark.parametrize('S', Cs.LL_MODELS)
def test_loglik_models_clamp_and_second_model(S):
    """n_models 1, 2, 5 with d_model = -3, 0, S - 1, S + 5 (clamped to [0, S)); max_frames = 33: the second tile has
    n_out = 1 and the length 70 is clamped to 33; the second model NULL, and equal to the first: ll_b == ll_a bit for bit."""
    poison_gpu_state()
    D, M = 8, 65
    c = Cs.ll_case(D, M, S, 33)
    assert c['eff'][-1] == 33
    raw, eff = Cs.ll_model_index(S)
    tab, _ = run_prepare(c['w'], c['mu'], c['var'])
    res = twice(lambda: run_loglik(c['x'], c['lens'], tab, S, M, raw, raw), 'second model equal to the first')
    only = twice(lambda: run_loglik(c['x'], c['lens'], tab, S, M, raw, None), 'second model NULL')
    clamped = run_loglik(c['x'], c['lens'], tab, S, M, eff, None)
    assert np.array_equal(res['ll_b'], res['ll_a']) and np.array_equal(only['ll_a'], res['ll_a']) and np.array_equal(clamped['ll_a'], res['ll_a'])
    worst = _ll_check(c, res['ll_a'], eff, 'clamped models')
    assert measured('vc_gmm_loglik_f32 n_models %d max_frames 33' % S, worst[1], worst[2]) <= 1.0
    if S > 1:                                                            # the models do differ: the clamp is observable
        other = run_loglik(c['x'], c['lens'], tab, S, M, [0] * len(raw), None)
        assert not np.array_equal(other['ll_a'], res['ll_a'])


def test_loglik_of_a_frame_depends_on_the_frame_and_model_alone():
    """One frame vector written at every position of a 70-frame row: all 70 ll have identical bits (every eight-frame group,
    every wave of the log-sum-exp, every tile)."""
    poison_gpu_state()
    D, M = 63, 193
    c = Cs.ll_case(D, M, 2, 70)
    x = np.full((2, 70 + Cs.PAD, D), np.nan, np.float32)
    x[0, :70] = c['x'][8, 3]
    x[1, :70] = c['x'][8, 69]                                            # the frame 40 sigma out
    tab, _ = run_prepare(c['w'], c['mu'], c['var'])
    res = twice(lambda: run_loglik(x, [70, 70], tab, 2, M, [0, 1], [1, 0]), 'one frame everywhere')
    for k in ('ll_a', 'll_b'):
        for b in (0, 1):
            assert (res[k][b, :70] == res[k][b, 0]).all(), (k, b)
            assert not res[k][b, 70:].any()
    assert res['ll_a'][0, 0] != res['ll_b'][0, 0] and res['ll_a'][0, 0] != res['ll_a'][1, 0]


# ================================================================================================ score
def _score_alone(a, b_, n, mask_u):
    if n == 0:
        return run_score(np.zeros((1, 1), np.float32), None if b_ is None else np.zeros((1, 1), np.float32), [0], None)
    return run_score(a[None, :n].copy(), None if b_ is None else b_[None, :n].copy(), [n],
                     None if mask_u is None else (mask_u[None, :n] != 0).astype(np.uint8))


@pytest.mark.parametrize('masked', ['null', 'random', 'none_kept'])
def test_score_integer_ll_is_exact(masked):
    """len 0, 1, 255, 256, 257, 513 (a lane's second and third trip): integer ll make every sum exact, so the figures are
    float32(sum / n) and the rounded float64 difference, bit for bit; NaN figures without a kept frame; ll_b NULL."""
    poison_gpu_state()
    a, b_, mask = Cs.score_batch(True)
    F = a.shape[1]
    if masked == 'null':
        mask = None
    elif masked == 'none_kept':
        mask = np.where(Cs.kept(Cs.SCORE_LENS, F), 0, 0xA5).astype(np.uint8)
    res = twice(lambda: run_score(a, b_, Cs.SCORE_LENS, mask), 'vc_gmm_score_f32')
    noref = twice(lambda: run_score(a, None, Cs.SCORE_LENS, mask), 'vc_gmm_score_f32, ll_b NULL')
    keep = Cs.kept(Cs.SCORE_LENS, F, mask)
    for u, n in enumerate(Cs.SCORE_LENS):
        cnt = int(keep[u].sum())
        assert res['n'][u] == cnt == noref['n'][u], (u, n)
        v, v0 = f32(res['values'])[u], f32(noref['values'])[u]
        assert np.isnan(v0[1]) and np.isnan(v0[2])
        if cnt == 0:
            assert np.isnan(v).all() and np.isnan(v0).all()
        else:
            sa, sb = float(a[u][keep[u]].astype(np.int64).sum()), float(b_[u][keep[u]].astype(np.int64).sum())
            want = np.array([sa / cnt, sb / cnt, sa / cnt - sb / cnt]).astype(np.float32)
            assert np.array_equal(res['values'][u], bits32(want)), (u, n, v, want)
            assert noref['values'][u, 0] == res['values'][u, 0]
        alone = _score_alone(a[u], b_[u], n, None if mask is None else mask[u])
        assert alone['n'][0] == res['n'][u] and np.array_equal(alone['values'][0], res['values'][u]), (u, 'alone against the batch')
    if masked == 'none_kept':
        assert not res['n'].any()
    if masked == 'null':
        assert res['n'].tolist() == Cs.SCORE_LENS


def test_score_real_ll_against_float64():
    poison_gpu_state()
    a, b_, mask = Cs.score_batch(False)
    res = twice(lambda: run_score(a, b_, Cs.SCORE_LENS, mask), 'vc_gmm_score_f32')
    worst = (0.0, 0.0, 0.0)
    for u, n in enumerate(Cs.SCORE_LENS):
        cnt, sa, sb, sl = sr.score(Cs.clean(a[u]), Cs.clean(b_[u]), n, mask[u])
        assert res['n'][u] == cnt
        if cnt == 0:
            assert np.isnan(f32(res['values'])[u]).all()
            continue
        keep = Cs.kept([n], a.shape[1], mask[u:u + 1])[0]
        ma, mb = float(np.abs(a[u][keep]).mean()), float(np.abs(b_[u][keep]).mean())
        for k, (ref, scale) in enumerate(((sa, ma), (sb, mb), (sl, ma + mb))):
            err, bound = abs(float(f32(res['values'])[u, k]) - ref), Cs.score_bound(ref, cnt, scale)
            assert err <= bound, (u, k, err, bound)
            worst = max(worst, (err / bound, err, bound))
        alone = _score_alone(a[u], b_[u], n, mask[u])
        assert np.array_equal(alone['values'][0], res['values'][u])
    assert measured('vc_gmm_score_f32 real ll', worst[1], worst[2]) <= 1.0


# ================================================================================================ accumulate
def _device_ll(c, tab, x=None):
    """The device's own ll under the case's model, on the host, with NaN behind every length."""
    x = c['x'] if x is None else x
    S = c['mu'].shape[0]
    M = c['mu'].shape[1]
    ll = f32(run_loglik(x, c['lens'], tab, S, M, [c.get('model', 0)] * len(c['lens']))['ll_a']).copy()
    for b, n in enumerate(c['lens']):
        ll[b, max(n, 0):] = np.nan
    return ll


def _exact_setup(c):
    """Table, the ll (asserted to be float32(c - q / 2), c read back from the table), and the float64 sum L per group."""
    tab, tbits = run_prepare(c['w'], c['mu'], c['var'])
    S, M, D = c['mu'].shape
    cm = f32(tbits[(S + 1) * M * D:])
    assert np.isneginf(np.delete(cm, c['m_star'])).all() and np.isfinite(cm[c['m_star']])
    ll = _device_ll(c, tab)
    L, A = np.zeros(c['G']), np.zeros(c['G'])
    for b, n in enumerate(c['lens']):
        want = Cs.exact_ll(cm[c['m_star']], c['x'][b, :n], c['mu'][c['model'], c['m_star']])
        assert np.array_equal(bits32(ll[b, :n]), bits32(want)), (c['name'], b, 'll is not float32(c - q / 2)')
        if 0 <= c['groups'][b] < c['G']:
            L[c['groups'][b]] += ll[b][c['keep'][b]].astype(np.float64).sum()
            A[c['groups'][b]] += np.abs(ll[b][c['keep'][b]].astype(np.float64)).sum()
    return tab, ll, L, A


def _check_exact(c, res, L, A, what):
    for k in ('N', 'S1', 'S2'):
        got = f64(res[k])
        assert not np.isnan(got).any(), (what, k, 'NaN')
        assert np.array_equal(got, c[k]), (what, k, np.argwhere(got != c[k])[:4].tolist())
    n_frames = int(c['N'].sum())
    err = np.abs(f64(res['L']) - L)
    assert (err <= Cs.l_bound(max(n_frames, 1)) * A).all(), (what, 'L', float(err.max()))
    return float(err.max()), float((Cs.l_bound(max(n_frames, 1)) * A).max())


@pytest.mark.parametrize('name', list(Cs.ACC_EXACT))
def test_accumulate_exact_sums(name):
    """One live component, integer features, unit variances: gamma is exactly 1 or 0, so N, S1 and S2 are integers in every
    partition geometry -- a tile dropped, doubled or sent to another group changes one.  The wrap cases (a partition's
    second step through an utterance), b >= P, the grid's z limit, groups left out and empty, the chunk and d = r + 4 j
    ownership over M x D, the muT offset of a 3-model table.  L against the float64 sum of the same ll."""
    poison_gpu_state()
    c = Cs.acc_exact(name)
    P = Cs.partitions(c['G'])
    print('CASE %s: G %d, P %d, (M, m*, D) = (%d, %d, %d); tiles reached by k += P: %s; utterances with b >= P: %s'
          % (name, c['G'], P, c['M'], c['m_star'], c['D'], (Cs.wrapped(c['lens'], c['groups'], c['G']) if P > 1 else [])[:6],
             [b for b in range(len(c['lens'])) if P > 1 and b >= P][:6]))
    tab, ll, L, A = _exact_setup(c)
    res = twice(lambda: run_accumulate(c['x'], ll, c['lens'], c['mask'], c['groups'], tab, c['S'], c['M'], c['model'], c['G']),
                'vc_gmm_accumulate_f32 ' + name)
    err, bound = _check_exact(c, res, L, A, name)
    measured('vc_gmm_accumulate_f32 %s L' % name, err, bound)
    empty = [g for g in range(c['G']) if g not in set(c['groups'])]
    assert bool(empty) == (c['G'] > 1)
    if empty:
        assert not res['N'][empty].any() and not res['S1'][empty].any() and not res['S2'][empty].any() and not res['L'][empty].any()


@pytest.mark.parametrize('name', ['b_ge_p2', 'wrap_p3', 'own_M65_D5', 'z_limit'])
def test_accumulate_counts_kept_frames_only(name):
    """A frame the mask drops contributes nothing, whatever it holds: +inf features and a NaN ll in every dropped frame
    (and NaN behind every length, as everywhere) leave the exact sums exact."""
    poison_gpu_state()
    c = Cs.acc_exact(name)
    tab, ll, L, A = _exact_setup(c)
    dropped = Cs.kept(c['lens'], c['F']) & ~c['keep']
    assert dropped.any()
    x, ll = c['x'].copy(), ll.copy()
    x[dropped] = np.inf
    ll[dropped] = np.nan
    res = twice(lambda: run_accumulate(x, ll, c['lens'], c['mask'], c['groups'], tab, c['S'], c['M'], c['model'], c['G']),
                'dropped frames hold inf and NaN')
    _check_exact(c, res, L, A, name + ', +inf in dropped frames')
    clean = run_accumulate(c['x'], _device_ll(c, tab), c['lens'], c['mask'], c['groups'], tab, c['S'], c['M'], c['model'], c['G'])
    for k in res:
        assert np.array_equal(res[k], clean[k]), k


@pytest.mark.parametrize('lo,hi', Cs.ACC_PAIRS)
def test_accumulate_workspace_path_against_direct_path(lo, hi):
    """The same inputs, groups in [0, 64), at G = 64 (two partitions, a workspace, the reduction launch) and G = 65 (one
    partition writes the outputs), and at 127 / 128 (one partition by the division and by the compare): bit-equal on the
    exact case; on real-valued data equal within the float64 summation order.  A NULL workspace of 0 bytes is accepted
    where the query returns 0."""
    poison_gpu_state()
    a, b_ = Cs.acc_exact('pair', lo), Cs.acc_exact('pair', hi)
    assert np.array_equal(bits32(a['x']), bits32(b_['x'])) and np.array_equal(a['mask'], b_['mask'])
    tab, ll, L, A = _exact_setup(a)
    ra = twice(lambda: run_accumulate(a['x'], ll, a['lens'], a['mask'], a['groups'], tab, 1, a['M'], 0, lo), 'G %d' % lo)
    rb = twice(lambda: run_accumulate(a['x'], ll, a['lens'], a['mask'], a['groups'], tab, 1, a['M'], 0, hi, null_ws=True), 'G %d' % hi)
    _check_exact(a, ra, L, A, 'G %d' % lo)
    for k in ra:
        assert np.array_equal(ra[k][:lo], rb[k][:lo]) and not rb[k][lo:].any(), (k, 'exact case: workspace path against direct path')
    # real-valued
    r = Cs.real_case(5, 256)
    groups = [0, 63, 5, 63, 0, 17]
    tabr, _ = run_prepare(r['w'], r['mu'], r['var'])
    llr = _device_ll(r, tabr)
    qa = run_accumulate(r['x'], llr, r['lens'], r['mask'], groups, tabr, 2, 256, 0, lo)
    qb = run_accumulate(r['x'], llr, r['lens'], r['mask'], groups, tabr, 2, 256, 0, hi, null_ws=True)
    ref = sr.accumulate(Cs.clean(r['x']), r['lens'], groups, lo, r['w'], r['mu'][0], r['var'], r['mask'])
    keep = Cs.kept(r['lens'], r['F'], r['mask'])
    absL = np.zeros(lo)
    for b, g in enumerate(groups):
        absL[g] += np.abs(llr[b][keep[b]].astype(np.float64)).sum()
    frames, worst = int(keep.sum()), 0.0
    for k, scale in (('N', ref['N']), ('S1', ref['A1']), ('S2', ref['S2']), ('L', absL)):
        err = np.abs(f64(qa[k]) - f64(qb[k])[:lo])
        bound = Cs.order_bound(frames, Cs.partitions(lo), scale * (1 + 1e-3))          # (the reference's own sums as the scale)
        assert (err <= bound).all(), (k, float(err.max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert not qb[k][lo:].any()
    print('MEASURED vc_gmm_accumulate_f32 G %d against G %d, real-valued err/bound=%.3f' % (lo, hi, worst))
    if Cs.partitions(lo) == 1:
        for k in qa:
            assert np.array_equal(qa[k], qb[k][:lo]), k                  # one partition on both sides: the same order


def test_accumulate_adds_in_the_documented_order():
    """N bit for bit on real-valued data.  The responsibilities themselves come from the device: every frame as an
    utterance of its own in a group of its own (one partition, one addition to 0.0) returns its float32 gamma widened.
    The same frames in their utterances must then give, per group and component, the float64 sum in the header's order:
    tile k of utterance b in partition (b + k) mod P, utterances and tiles ascending, frames ascending, partitions
    0 .. P - 1."""
    poison_gpu_state()
    c = Cs.ORDER_CASE
    G, D, M, lens, groups = c['G'], c['D'], c['M'], c['lens'], c['groups']
    r = Cs.real_case(D, M)
    rng = np.random.RandomState(12)
    F = max(lens) + Cs.PAD
    x = np.full((len(lens), F, D), np.nan, np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = r['x'][4, rng.randint(4, 69, n)]                     # frames of hard_case off its narrow component
    mask = Cs.random_mask(rng, lens, F, 0.8)
    keep = Cs.kept(lens, F, mask)
    tab, _ = run_prepare(r['w'], r['mu'], r['var'])
    case = dict(x=x, lens=lens, mu=r['mu'])
    ll = _device_ll(case, tab)
    rows = [(b, f) for b, n in enumerate(lens) for f in range(n)]
    one_x = np.stack([x[b, f] for b, f in rows])[:, None, :]
    one_ll = np.array([ll[b, f] for b, f in rows], np.float32)[:, None]
    single = run_accumulate(one_x, one_ll, [1] * len(rows), None, list(range(len(rows))), tab, 2, M, 0, len(rows))
    assert Cs.partitions(len(rows)) == 1
    gamma = np.zeros((len(lens), F, M))
    for i, (b, f) in enumerate(rows):
        gamma[b, f] = f64(single['N'])[i]
    assert (gamma >= 0).all() and abs(gamma.sum() - len(rows)) <= 1e-4 * len(rows) and len(np.unique(gamma)) > len(rows)
    res = twice(lambda: run_accumulate(x, ll, lens, mask, groups, tab, 2, M, 0, G), 'the order case')
    want = Cs.ordered_sum(gamma, keep, lens, groups, G)
    assert np.array_equal(f64(res['N']), want), np.argwhere(f64(res['N']) != want)[:4].tolist()


@pytest.mark.parametrize('D,M,G', Cs.ACC_REAL)
def test_accumulate_real_valued_two_delta_rule(D, M, G):
    """test_accumulate_against_float64 of tests/test_speaker_gpu.py, in dirty buffers with a mask: gamma carries the error
    of l_m and of ll, at most delta each, so N is off by at most 2 delta N, S1 by 2 delta sum gamma |x|, S2 by 2 delta S2,
    L by delta max(N, 1); right-hand sides from the float64 reference."""
    poison_gpu_state()
    c = Cs.real_case(D, M)
    groups = [b % min(G, 3) if G > 1 else 0 for b in range(len(c['lens']))]
    groups[3] = -1 if G > 1 else 0
    tab, _ = run_prepare(c['w'], c['mu'], c['var'])
    ll = _device_ll(c, tab)
    res = twice(lambda: run_accumulate(c['x'], ll, c['lens'], c['mask'], groups, tab, 2, M, 0, G), 'real-valued')
    want = sr.accumulate(Cs.clean(c['x']), c['lens'], groups, G, c['w'], c['mu'][0], c['var'], c['mask'])
    delta = max(float(bd.max()) for b, (_, bd) in enumerate(Cs.real_ll(D, M)) if 0 <= groups[b] < G)
    tiny = 1e-300
    rN = np.abs(f64(res['N']) - want['N']) / (2 * delta * want['N'] + tiny)
    r1 = np.abs(f64(res['S1']) - want['S1']) / (2 * delta * want['A1'] + tiny)
    r2 = np.abs(f64(res['S2']) - want['S2']) / (2 * delta * want['S2'] + tiny)
    rL = np.abs(f64(res['L']) - want['L']) / (delta * np.maximum(want['N'].sum(1), 1.0))
    for what, r in (('N', rN), ('S1', r1), ('S2', r2), ('L', rL)):
        print('MEASURED vc_gmm_accumulate_f32 D%d M%d G%d %s err/bound=%.3f' % (D, M, G, what, float(r.max())))
        assert r.max() <= 1.0, (what, float(r.max()))
    keep = Cs.kept(c['lens'], c['F'], c['mask'])
    n_kept = sum(int(keep[b].sum()) for b, g in enumerate(groups) if 0 <= g < G)
    assert abs(float(f64(res['N']).sum()) - n_kept) <= 1e-4 * n_kept


def test_accumulate_refuses_a_short_or_unaligned_workspace_and_writes_nothing():
    poison_gpu_state()
    lib, st = _lib(), _st()
    c = Cs.acc_exact('own_M65_D5')
    tab, _ = run_prepare(c['w'], c['mu'], c['var'])
    B, F, D, M, G = len(c['lens']), c['F'], c['D'], c['M'], c['G']
    need = lib.vc_gmm_workspace_bytes(G, M, D)
    assert need > 0 and need % 256 == 0
    d_x, d_ll, d_len, d_g = dev(Cs.clean(c['x'])), dev(np.zeros((B, F), np.float32)), i32(c['lens']), i32(c['groups'])
    ws = Buf(need + 8, 'b')
    N, S1, S2, L = Buf(G * M, 'd'), Buf(G * M * D, 'd'), Buf(G * M * D, 'd'), Buf(G, 'd')

    def call(off=0, size=need, p=True):
        return lib.vc_gmm_accumulate_f32(ptr(d_x), ptr(d_ll), ptr(d_len), None, ptr(d_g), B, F, D, tab.ptr(), 1, M, 0, G, N.ptr(), S1.ptr(),
                                         S2.ptr(), L.ptr(), ws.ptr(off) if p else None, size, st)

    _refused(call(size=need - 1), VC_ERR_WORKSPACE, 'workspace')
    _refused(call(off=4), VC_ERR_INVALID, 'unaligned')
    _refused(call(off=1), VC_ERR_INVALID, 'unaligned')
    _refused(call(p=False), VC_ERR_INVALID, 'workspace')
    assert all(b.untouched() for b in (ws, N, S1, S2, L))
    _ok(call(off=8))                                                      # 8-byte alignment is what the launch asks for
    assert ws.bands_ok()
    N.bits(), S1.bits(), S2.bits(), L.bits()


def test_lengths_outside_their_range_are_clamped_in_all_four_launches():
    """include/vc_hip.h: a d_len outside [0, max_frames], of any magnitude, is clamped: -7, max_frames + 100 and 0x7fffffff
    give the bits of 0, max_frames and max_frames in vc_spk_features_f32, vc_gmm_loglik_f32, vc_gmm_score_f32 and
    vc_gmm_accumulate_f32."""
    poison_gpu_state()
    F, D, M = 37, 4, 65
    raw, eff = [-7, F + 100, IFILL, 5], [0, F, F, 5]
    rng = np.random.RandomState(77)
    cep = rng.randint(-8, 9, (4, F, 2)).astype(np.float32)
    mask = (rng.rand(4, F) < 0.7).astype(np.uint8)
    got, want = {}, {}
    for lens, store in ((raw, got), (eff, want)):
        store['feat'] = run_features(cep, lens, mask, 1, 1)['feat']
    c = Cs.acc_exact('own_M65_D4')
    x = rng.randint(-3, 4, (4, F, D)).astype(np.float32)
    tab, _ = run_prepare(c['w'], c['mu'], c['var'])
    for lens, store in ((raw, got), (eff, want)):
        store.update(run_loglik(x, lens, tab, 1, M, [0] * 4))
        ll = f32(store['ll_a']).copy()
        store.update(run_score(ll, ll, lens, mask))
        store.update(run_accumulate(x, ll, lens, mask, [0, 2, 0, 2], tab, 1, M, 0, 3))
    assert set(got) == {'feat', 'll_a', 'n', 'values', 'N', 'S1', 'S2', 'L'}
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    assert want['n'].tolist() == [0] + [int(mask[b, :n].sum()) for b, n in list(enumerate(eff))[1:]]
    assert f64(want['N'])[:, 64].tolist() == [float(want['n'][0] + want['n'][2]), 0.0, float(want['n'][1] + want['n'][3])]


# ================================================================================================ update
@pytest.mark.parametrize('M,D', Cs.UPDATE_EM_SHAPES)
def test_update_em(M, D):
    """M D = 255, 256, 258 and 256 x 64 (the last block partly filled); zero occupancy; N just below and at min_count; the
    floor binding in one dimension only; within the project's 2 float32 ulp of the float64 reference."""
    poison_gpu_state()
    N, mean, v, mu_old, var_old = (a.copy() for a in Cs.update_stats(1, M, D))
    N[0, 3] = 0.0
    N[0, 4] = np.nextafter(1.0, 0.0)                                     # just below min_count: the old values stay
    N[0, 5] = 1.0                                                        # at min_count: updated
    v[0, 6, 2] = 1e-5                                                    # the floor binds in one dimension only
    S1, S2 = mean * N[..., None], (v + mean * mean) * N[..., None]
    floor = np.full(D, 0.01, np.float32)
    res = twice(lambda: run_update(0, N, S1, S2, mu_old, var_old, floor, 1.0, 0.0), 'vc_gmm_update_f32 EM')
    w, mu, var = f32(res['w']), f32(res['mu'])[0], f32(res['var'])
    ww, wm, wv = sr.update_em(N[0], S1[0], S2[0], mu_old, var_old, floor, 1.0)
    worst = max(float(ulps(w, ww).max()), float(ulps(mu, wm).max()), float(ulps(var, wv).max()))
    assert measured('vc_gmm_update_f32 EM %dx%d (ulp)' % (M, D), worst, Cs.UPDATE_ULPS) <= 1.0
    assert np.array_equal(bits32(mu[3:5]), bits32(mu_old[3:5])) and np.array_equal(bits32(var[3:5]), bits32(var_old[3:5]))
    assert not np.array_equal(bits32(mu[5]), bits32(mu_old[5])) and float(ulps(mu[5], mean[0, 5].astype(np.float32)).max()) <= 2.0
    assert w[3] == np.float32(2.0 ** -40) and var[6, 2] == np.float32(0.01) and (np.delete(var[6], 2) > 0.1).all()


def test_update_em_without_a_frame_keeps_the_model_and_floors_every_weight():
    poison_gpu_state()
    M, D = 65, 5
    _, _, _, mu_old, var_old = Cs.update_stats(1, M, D)
    z = np.zeros((1, M))
    res = twice(lambda: run_update(0, z, np.zeros((1, M, D)), np.zeros((1, M, D)), mu_old, var_old, np.full(D, 0.01, np.float32), 1.0, 0.0),
                'all N zero')
    assert (f32(res['w']) == np.float32(2.0 ** -40)).all()
    assert np.array_equal(res['mu'][0], bits32(mu_old)) and np.array_equal(res['var'], bits32(var_old))


def test_update_em_variance_under_cancellation():
    """A variance of 1e-3 under a squared mean of 1e6: S2 / n - mean^2 loses nine digits in float64.  Bound: half a float32
    ulp plus 4 2^-53 (S2 / n + mean^2), against the exact rational value; holds fused or not (the CPU file)."""
    poison_gpu_state()
    n, S1, S2 = Cs.cancellation_case()
    true, bound = Cs.cancellation_bound(n, S1, S2)
    res = twice(lambda: run_update(0, np.array([[n]]), np.array([[[S1]]]), np.array([[[S2]]]), np.zeros((1, 1), np.float32),
                                   np.ones((1, 1), np.float32), np.full(1, 1e-12, np.float32), 1.0, 0.0), 'cancellation')
    got = float(f32(res['var'])[0, 0])
    assert measured('vc_gmm_update_f32 variance under cancellation', abs(got - true), bound) <= 1.0
    assert f32(res['mu'])[0, 0, 0] == np.float32(S1 / n) and f32(res['w'])[0] == 1.0


@pytest.mark.parametrize('G,M,D', [(1, 65, 5), (3, 64, 4), (4096, 5, 3), Cs.UPDATE_MAP_257])
def test_update_map(G, M, D):
    """MAP with 1, 3 and 4,096 groups and G M D = 257; rows with N = 0 return mu_in bit for bit; relevance 0 is alpha = 1:
    the group's own mean; the pointers the mode does not read may be NULL."""
    poison_gpu_state()
    N, mean, v, mu_old, var_old = (a.copy() for a in Cs.update_stats(G, M, D))
    if G > 1:
        N[G // 2] = 0.0                                                  # a group without a frame
    N[0, M - 1] = 0.0
    S1 = mean * N[..., None]
    res = twice(lambda: run_update(1, N, S1, None, mu_old, None, None, 0.0, 16.0, nulls=True), 'vc_gmm_update_f32 MAP')
    full = run_update(1, N, S1, S1, mu_old, var_old, np.ones(D, np.float32), 0.0, 16.0)
    assert np.array_equal(full['mu'], res['mu'])
    got = f32(res['mu'])
    want = sr.update_map(N, S1, mu_old, 16.0)
    assert measured('vc_gmm_update_f32 MAP G%d %dx%d (ulp)' % (G, M, D), float(ulps(got, want).max()), Cs.UPDATE_ULPS) <= 1.0
    assert np.array_equal(res['mu'][0, M - 1], bits32(mu_old[M - 1])) and (G == 1 or np.array_equal(res['mu'][G // 2], bits32(mu_old)))
    zero = run_update(1, N, S1, None, mu_old, None, None, 0.0, 0.0, nulls=True)
    own = (S1 / np.where(N > 0, N, 1.0)[..., None]).astype(np.float32)
    live = N > 0
    assert live.any() and np.array_equal(zero['mu'][live], bits32(own[live])) and np.array_equal(zero['mu'][0, M - 1], bits32(mu_old[M - 1]))
