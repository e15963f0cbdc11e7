"""Intelligibility scoring on the MI355X: vc_stoi_energy_f32, vc_stoi_keep_f32, vc_stoi_bands_f32, vc_stoi_score_f32 and
vc_si_sdr_f32 alone through the C ABI against tests/stoi_ref.py, each on the device's own inputs to that stage; identity
alone / in a batch of four / under graph replay; evaluation.stoi_batch and si_sdr_batch end to end.

Every kernel call as tests/test_denoise_gpu.py makes them: every buffer inside sentinel bands that are checked after the
call, outputs filled with NaN (integers: with the NaN's bit pattern), waveform samples at or beyond an utterance's length NaN."""
import functools

import numpy as np
import pytest
import torch

from conftest import poison_gpu_state
import stoi_cases as sc
import stoi_ref as sr

pytestmark = pytest.mark.gpu

BAND = 1024
SENT = np.float32(-98765.4375)
NAN = float('nan')
NAN_I32 = int(np.float32(NAN).view(np.int32))
RATIO = float(np.float32(1e-4))
TAB = sr.bands()
NB = len(TAB)
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _poisoned():
    poison_gpu_state()


class Guarded:
    """n float32 (or int32 through .ints()) inside a larger device buffer whose bands hold the sentinel; .t is the inner view."""

    def __init__(self, n, fill=float(SENT), host=None):
        self.full = torch.full((n + 2 * BAND,), float(SENT), dtype=torch.float32, device='cuda')
        self.t = self.full[BAND:BAND + n]
        if host is not None:
            h = np.ascontiguousarray(host).reshape(-1)
            if h.dtype.kind in 'iu':
                self.t.view(torch.int32).copy_(torch.from_numpy(h.astype(np.int32)))
            else:
                self.t.copy_(torch.from_numpy(h.astype(np.float32)))
        elif fill != float(SENT):
            self.t.fill_(fill)

    def check(self, what):
        assert bool((self.full[:BAND] == float(SENT)).all()) and bool((self.full[-BAND:] == float(SENT)).all()), \
            'sentinel band overwritten around ' + what

    def numpy(self):
        return self.t.cpu().numpy()

    def ints(self):
        return self.t.cpu().numpy().view(np.int32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _measured(what, got, want, bound):
    """One MEASURED line for the element with the worst error / bound; an element whose bound is 0 must be exact."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape and got.size > 0, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what + ': the device value is not finite'
    err = np.abs(got - want)
    zero = bound <= 0.0
    assert not err[zero].any(), what + ': an element with bound 0 is not exact'
    if zero.all():
        print('MEASURED %s: error 0 bound 0 ratio 0.000 (all exact)' % what)
        return 0.0
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print('MEASURED %s: error %.3e bound %.3e ratio %.3f' % (what, err[i], bound[i], ratio[i]))
    assert ratio[i] <= 1.0, '%s: error %.3e > bound %.3e at %s' % (what, err[i], bound[i], i)
    return float(ratio[i])


def _dev_i32(v):
    return None if v is None else torch.tensor(list(v), dtype=torch.int32, device='cuda')


def _ptr(g):
    import _vc
    return None if g is None else _vc.ptr(g.t if isinstance(g, Guarded) else g)


def _finish(*named):
    torch.cuda.synchronize()
    for g, what in named:
        if g is not None:
            g.check(what)


# ------------------------------------------------------------------------------------------ one call of each launch
def _energy_call(wav, lens, maxF, null=None, batch=None, max_len=None, ld=None, max_frames=None):
    """(rc, e [B, maxF], frame counts int32 [B]); NaN / NaN's bits where the device wrote nothing."""
    import _vc
    B, L = wav.shape
    d_x, d_e, d_n = Guarded(wav.size, host=wav), Guarded(B * maxF, fill=NAN), Guarded(B, fill=NAN)
    p = dict(ref=_ptr(d_x), energy=_ptr(d_e), nf=_ptr(d_n))
    if null:
        p[null] = None
    rc = _vc.lib().vc_stoi_energy_f32(p['ref'], _ptr(_dev_i32(lens)), B if batch is None else batch, L if max_len is None else max_len,
                                      L if ld is None else ld, p['energy'], p['nf'], maxF if max_frames is None else max_frames,
                                      _vc.current_stream())
    _finish((d_x, 'd_ref'), (d_e, 'd_energy'), (d_n, 'd_n_frames'))
    assert _same_bits(d_x.numpy(), np.asarray(wav, np.float32).reshape(-1)), 'the waveform was written'
    return rc, d_e.numpy().reshape(B, maxF), d_n.ints()


def _keep_call(e, nf, ratio=RATIO, null=None, batch=None, max_frames=None):
    """(rc, idx int32 [B, maxF], K int32 [B])."""
    import _vc
    B, maxF = e.shape
    d_e, d_n, d_i, d_k = Guarded(e.size, host=e), Guarded(B, host=np.asarray(nf, np.int32)), Guarded(e.size, fill=NAN), Guarded(B, fill=NAN)
    p = dict(energy=_ptr(d_e), nf=_ptr(d_n), index=_ptr(d_i), kept=_ptr(d_k))
    if null:
        p[null] = None
    rc = _vc.lib().vc_stoi_keep_f32(p['energy'], p['nf'], B if batch is None else batch, maxF if max_frames is None else max_frames,
                                    ratio, p['index'], p['kept'], _vc.current_stream())
    _finish((d_e, 'd_energy'), (d_n, 'd_n_frames'), (d_i, 'd_index'), (d_k, 'd_n_kept'))
    return rc, d_i.ints().reshape(B, maxF), d_k.ints()


def _bands_call(ref, deg, idx, K, max_m, tab=TAB, null=None, batch=None, max_len=None, n_bands=None, max_frames=None, mm=None):
    """(rc, T [2, B, max_m, nb])."""
    import _vc
    B, L = ref.shape
    maxF, nb = idx.shape[1], len(tab)
    d_x, d_y = Guarded(ref.size, host=ref), Guarded(deg.size, host=deg)
    d_i, d_k, d_b = Guarded(idx.size, host=idx.astype(np.int32)), Guarded(B, host=np.asarray(K, np.int32)), Guarded(2 * nb, host=np.asarray(tab, np.int32))
    d_T = Guarded(2 * B * max_m * nb, fill=NAN)
    p = dict(ref=_ptr(d_x), deg=_ptr(d_y), index=_ptr(d_i), kept=_ptr(d_k), bands=_ptr(d_b), T=_ptr(d_T))
    if null:
        p[null] = None
    rc = _vc.lib().vc_stoi_bands_f32(p['ref'], p['deg'], B if batch is None else batch, L if max_len is None else max_len, L, p['index'],
                                     p['kept'], maxF if max_frames is None else max_frames, p['bands'], nb if n_bands is None else n_bands,
                                     p['T'], max_m if mm is None else mm, _vc.current_stream())
    _finish((d_x, 'd_ref'), (d_y, 'd_deg'), (d_i, 'd_index'), (d_k, 'd_n_kept'), (d_b, 'd_bands'), (d_T, 'd_T'))
    assert _same_bits(d_x.numpy(), np.asarray(ref, np.float32).reshape(-1)) and _same_bits(d_y.numpy(), np.asarray(deg, np.float32).reshape(-1))
    return rc, d_T.numpy().reshape(2, B, max_m, nb)


def _score_call(T, K, maxF, mode, max_seg, null=None, batch=None, n_bands=None, mm=None, ms=None):
    """(rc, seg [B, max_seg], score [B], n_segments int32 [B])."""
    import _vc
    _, B, max_m, nb = T.shape
    d_T, d_k = Guarded(T.size, host=T), Guarded(B, host=np.asarray(K, np.int32))
    d_g, d_s, d_n = Guarded(B * max_seg, fill=NAN), Guarded(B, fill=NAN), Guarded(B, fill=NAN)
    p = dict(T=_ptr(d_T), kept=_ptr(d_k), seg=_ptr(d_g), score=_ptr(d_s), nseg=_ptr(d_n))
    if null:
        p[null] = None
    rc = _vc.lib().vc_stoi_score_f32(p['T'], p['kept'], B if batch is None else batch, maxF, max_m if mm is None else mm,
                                     nb if n_bands is None else n_bands, mode, p['seg'], max_seg if ms is None else ms, p['score'],
                                     p['nseg'], _vc.current_stream())
    _finish((d_T, 'd_T'), (d_k, 'd_n_kept'), (d_g, 'd_seg'), (d_s, 'd_score'), (d_n, 'd_n_segments'))
    assert _same_bits(d_T.numpy(), T.reshape(-1)), 'T was written'
    return rc, d_g.numpy().reshape(B, max_seg), d_s.numpy(), d_n.ints()


def _si_call(ref, deg, lens, zero_mean, null=None, batch=None, max_len=None, ld=None):
    """(rc, si_sdr [B], valid uint8 [B])."""
    import _vc
    B, L = ref.shape
    d_x, d_y, d_s = Guarded(ref.size, host=ref), Guarded(deg.size, host=deg), Guarded(B, fill=NAN)
    d_v = torch.full((B + 2 * BAND,), 0xA5, dtype=torch.uint8, device='cuda')
    p = dict(ref=_ptr(d_x), deg=_ptr(d_y), out=_ptr(d_s), valid=_ptr(d_v[BAND:BAND + B]))
    if null:
        p[null] = None
    rc = _vc.lib().vc_si_sdr_f32(p['ref'], p['deg'], _ptr(_dev_i32(lens)), B if batch is None else batch, L if max_len is None else max_len,
                                 L if ld is None else ld, zero_mean, p['out'], p['valid'], _vc.current_stream())
    _finish((d_x, 'd_ref'), (d_y, 'd_deg'), (d_s, 'd_si_sdr'))
    v = d_v.cpu().numpy()
    assert (v[:BAND] == 0xA5).all() and (v[-BAND:] == 0xA5).all(), 'sentinel band overwritten around d_valid'
    return rc, d_s.numpy(), v[BAND:BAND + B]


def _chain_to_T(ref, deg, lens):
    """energy, keep and bands on the device: (e, nf, idx, K, T, maxF, max_m)."""
    maxF = max(sr.n_frames(ref.shape[1]), 1)
    max_m = max(maxF - 1, 1)
    rc, e, nf = _energy_call(ref, lens, maxF)
    assert rc == 0
    rc, idx, K = _keep_call(e, nf)
    assert rc == 0
    rc, T = _bands_call(ref, deg, idx, K, max_m)
    assert rc == 0
    return e, nf, idx, K, T, maxF, max_m


@functools.lru_cache(maxsize=None)
def _band_reference(name):
    x, y = sc.band_case(name)
    idx = sr.kept(sr.energies(x))
    return idx, sr.band_T(x, idx), sr.band_T(y, idx), sr.band_bound(x, idx), sr.band_bound(y, idx)


# ------------------------------------------------------------------------------------------ energy and the kept list
def _check_energy_and_list(tag, wav, lens, e, nf, idx, K):
    B, maxF = e.shape
    for b in range(B):
        n = wav.shape[1] if lens is None else min(max(int(lens[b]), 0), wav.shape[1])
        want = sr.energies(np.nan_to_num(wav[b]), n)
        F = len(want)
        assert int(nf[b]) == F == sr.n_frames(n), (tag, b, int(nf[b]), F)
        assert not np.isnan(e[b]).any() and not e[b, F:].any(), '%s utt %d: a row at or beyond F is not 0' % (tag, b)
        if F:
            # 256 terms (x w)^2: w within u, the product and the square rounded (4 u on a term), sums of 4 and of 64
            _measured('energy %s utt %d (len %d, F %d)' % (tag, b, n, F), e[b, :F], want, (4 + 4 + 6) * U * want)
        keep = sr.kept(want)
        assert int(K[b]) == len(keep), (tag, b, int(K[b]), len(keep))
        assert idx[b, :len(keep)].tolist() == keep.tolist() and (idx[b, len(keep):] == -1).all(), '%s utt %d: the kept list differs' % (tag, b)


def test_energy_and_kept_list_are_exact_on_the_ragged_batch():
    """L in {0, 256, 257, 384, 385, 4000}, digital silence, and a quiet lead, interior gap and tail, in one batch with NaN
    beyond every length: frame counts, kept list and K exact (tests/test_stoi_cpu.py shows every threshold 1e-3 away), the
    energies within float32 rounding.  Digital silence keeps nothing.  lens NULL, below and equal to Lmax."""
    wav, lens = sc.energy_batch()
    maxF = sr.n_frames(wav.shape[1])
    rc, e, nf = _energy_call(wav, lens, maxF)
    assert rc == 0
    rc, idx, K = _keep_call(e, nf)
    assert rc == 0
    _check_energy_and_list('ragged', wav, lens, e, nf, idx, K)
    assert K[:4].tolist() == [0, 0, 1, 1] and int(K[6]) == 0 and int(nf[6]) == sr.n_frames(4000)
    assert (np.diff(idx[7, :K[7]]) > 1).any() and idx[7, 0] > 0
    # one more row than any utterance has frames, junk lengths clamped
    clean = np.where(np.isnan(wav), 0.05, wav)
    junk = [-5, 10 ** 9, 257, 384, 385, 4000, 4000, wav.shape[1]]
    rc, e2, nf2 = _energy_call(clean, junk, maxF + 1)
    assert rc == 0
    rc, idx2, K2 = _keep_call(e2, nf2)
    assert rc == 0
    _check_energy_and_list('junk-and-equal', clean, junk, e2, nf2, idx2, K2)
    rc, e3, nf3 = _energy_call(clean, None, maxF)
    assert rc == 0 and (nf3 == maxF).all()
    rc, idx3, K3 = _keep_call(e3, nf3)
    assert rc == 0
    _check_energy_and_list('null', clean, None, e3, nf3, idx3, K3)
    # frame counts from memory are clamped too
    rc, idx4, K4 = _keep_call(e3, [-3, maxF + 9] + [maxF] * 6)
    assert rc == 0 and int(K4[0]) == 0 and (idx4[0] == -1).all() and idx4[1].tolist() == idx3[1].tolist()


def test_refusals_launch_nothing():
    import _vc
    err = _vc.lib().vc_last_error
    wav, lens = sc.energy_batch()
    wav = wav[2:6, :4100]
    lens = lens[2:6]
    maxF = sr.n_frames(wav.shape[1])
    for kw in (dict(null='ref'), dict(null='energy'), dict(null='nf'), dict(batch=0), dict(batch=65536), dict(max_len=0), dict(ld=4099),
               dict(max_frames=0), dict(max_frames=maxF - 1), dict(max_frames=16385)):
        rc, e, nf = _energy_call(wav, lens, maxF, **kw)
        assert rc == 1 and b'vc_stoi_energy_f32' in err() and np.isnan(e).all() and (nf == NAN_I32).all(), kw
    rc, e, nf = _energy_call(wav, lens, maxF)
    for kw in (dict(null='energy'), dict(null='nf'), dict(null='index'), dict(null='kept'), dict(batch=0), dict(max_frames=0),
               dict(max_frames=16385), dict(ratio=0.0), dict(ratio=1.0), dict(ratio=NAN)):
        rc, idx, K = _keep_call(e, nf, **kw)
        assert rc == 1 and b'vc_stoi_keep_f32' in err() and (idx == NAN_I32).all() and (K == NAN_I32).all(), kw
    rc, idx, K = _keep_call(e, nf)
    clean = np.nan_to_num(wav)
    for kw in (dict(null='ref'), dict(null='deg'), dict(null='index'), dict(null='kept'), dict(null='bands'), dict(null='T'),
               dict(batch=0), dict(max_len=0), dict(n_bands=0), dict(n_bands=33), dict(max_frames=0), dict(mm=0), dict(mm=16385)):
        rc, T = _bands_call(clean, clean, idx, K, maxF - 1, **kw)
        assert rc == 1 and b'vc_stoi_bands_f32' in err() and np.isnan(T).all(), kw
    T = np.zeros((2, 4, maxF - 1, NB), np.float32)
    for kw in (dict(null='T'), dict(null='kept'), dict(null='seg'), dict(null='score'), dict(null='nseg'), dict(batch=0),
               dict(n_bands=33), dict(mm=0), dict(ms=0), dict(mode=2), dict(mode=-1)):
        mode = kw.pop('mode', 0)
        rc, seg, s, n = _score_call(T, K, maxF, mode, 2, **kw)
        assert rc == 1 and b'vc_stoi_score_f32' in err() and np.isnan(seg).all() and np.isnan(s).all() and (n == NAN_I32).all(), kw
    for kw in (dict(null='ref'), dict(null='deg'), dict(null='out'), dict(null='valid'), dict(batch=0), dict(max_len=0), dict(ld=1),
               dict(zero_mean=2)):
        zm = kw.pop('zero_mean', 1)
        rc, s, v = _si_call(clean, clean, lens, zm, **kw)
        assert rc == 1 and b'vc_si_sdr_f32' in err() and np.isnan(s).all() and (v == 0xA5).all(), kw


# ------------------------------------------------------------------------------------------ bands
def test_bands_against_float64_on_every_case():
    """K in {1, 2, 3, 5, 16, 17, 18, 31} (M = 0, 1, 2, 4, 15, 16, 17, 30: below, at and above seams of the four-frame tile -- M = 4 and
    M = 16 leave whole live tiles followed by all-zero ones --, and partial last tiles), an impulse and a
    bin-centred cosine (closed forms: tests/test_stoi_cpu.py), the gather across non-adjacent frames; all in ONE ragged batch
    with NaN beyond each length, on the device's own kept list.  Against float64 (numpy's FFT of the materialised
    silence-removed signal) with the float32 model's bound; rows at or beyond M are 0; each utterance alone gives the same
    bits."""
    cases = [sc.band_case(c) for c in sc.BAND_CASES]
    lens = [len(x) for x, _ in cases]
    Lmax = max(lens) + 7
    ref, deg = np.full((len(cases), Lmax), NAN), np.full((len(cases), Lmax), NAN)
    for b, (x, y) in enumerate(cases):
        ref[b, :lens[b]], deg[b, :lens[b]] = x, y
    e, nf, idx, K, T, maxF, max_m = _chain_to_T(ref, deg, lens)
    assert not np.isnan(T).any()
    for b, name in enumerate(sc.BAND_CASES):
        keep, Tx, Ty, bx, by = _band_reference(name)
        M = max(len(keep) - 1, 0)
        assert int(K[b]) == len(keep) and idx[b, :len(keep)].tolist() == keep.tolist(), name
        assert not T[:, b, M:].any(), name + ': a row at or beyond M is not 0'
        if M:
            _measured('bands %s reference (K %d)' % (name, len(keep)), T[0, b, :M], Tx, bx)
            _measured('bands %s processed (K %d)' % (name, len(keep)), T[1, b, :M], Ty, by)
        one = _chain_to_T(ref[b:b + 1, :lens[b] + 1], deg[b:b + 1, :lens[b] + 1], [lens[b]])[4]
        assert _same_bits(one[:, 0, :M], T[:, b, :M]) and not one[:, 0, M:].any(), name + ': alone differs from the batch'
    x, p, A = sc.impulse()
    w = sr.window()
    b = sc.BAND_CASES.index('impulse')
    want = (w[168] + w[40]) * w[168] * A * np.sqrt(TAB[:, 1] - TAB[:, 0])
    _measured('bands impulse closed form', T[0, b, 0], want, _band_reference('impulse')[3][0])


def test_bands_take_the_table_and_the_list_as_they_are_given():
    """Another table (three bands, one empty, one reaching bin 256, out-of-range edges clamped) and a list that names frames
    the buffer cannot hold: those count as frames of zeros, nothing is read outside the waveform."""
    x, y = sc.band_case('K31')
    keep = _band_reference('K31')[0]
    tab = np.array([[0, 5], [40, 40], [200, 999]], np.int64)
    idx = np.full((1, 31), -1, np.int32)
    idx[0, :31] = keep
    rc, T = _bands_call(x[None], y[None], idx, [31], 30, tab=tab)
    assert rc == 0
    want = sr.band_T(x, keep, np.clip(tab, 0, 257))
    bound = sr.band_bound(x, keep, np.clip(tab, 0, 257))
    _measured('bands other table', T[0, 0], want, bound)
    assert not T[0, 0, :, 1].any()
    bad = idx.copy()
    bad[0, 3], bad[0, 9] = 10 ** 6, -7
    rc, T2 = _bands_call(x[None], y[None], bad, [31], 30)
    assert rc == 0 and np.isfinite(T2).all()
    rc, T1 = _bands_call(x[None], y[None], idx, [31], 30)
    untouched = [m for m in range(30) if not {m - 1, m, m + 1} & {3, 9}]
    assert _same_bits(T2[:, 0, untouched], T1[:, 0, untouched]) and not _same_bits(T2[:, 0, 3], T1[:, 0, 3])


# ------------------------------------------------------------------------------------------ score
@functools.lru_cache(maxsize=None)
def _score_T():
    ref, deg, lens = sc.score_batch()
    e, nf, idx, K, T, maxF, max_m = _chain_to_T(ref, deg, lens)
    assert K.tolist() == list(sc.SCORE_K)
    return T, K, maxF, max_m


def _variant(T, name):
    T = T.copy()
    if name == 'zero-y-band':
        T[1, :, :, 3] = 0.0
    elif name == 'zero-both':
        T[:, :, :, 7] = 0.0
    elif name == 'identical':
        T[1] = T[0]
    return T


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('variant', ('plain', 'zero-y-band', 'zero-both', 'identical'))
def test_score_against_the_restatement_on_the_devices_T(variant, mode):
    """M in {29, 30, 31} (S = 0, 1, 2) and {37, 38} (S = 8, 9: across the seam of the eight-segment tile) in one batch; a band
    that is zero in y, and in both; identical T.  The reference is the float64 restatement on the SAME T; the bound on seg
    and score is 4 x the largest distance between that and its float32 twin on the case.  Identical T: seg and score
    within a few float32 ulp of 1 (4 ulp of 2^-23 are allowed; the measured distance is printed)."""
    T0, K, maxF, max_m = _score_T()
    T = _variant(T0, variant)
    max_seg = max_m - sr.N_SEG + 1 + 1                              # one more row than any utterance has segments
    rc, seg, score, nseg = _score_call(T, K, maxF, mode, max_seg)
    assert rc == 0 and not np.isnan(seg).any()
    want_seg, twin_seg, want_score, twin_score = [], [], [], []
    for b, k in enumerate(sc.SCORE_K):
        M = k - 1
        a64 = sr.segments(T[0, b, :M], T[1, b, :M], mode)
        a32 = sr.segments(T[0, b, :M], T[1, b, :M], mode, np.float32)
        S = len(a64)
        assert int(nseg[b]) == S == max(M - sr.N_SEG + 1, 0) and not seg[b, S:].any(), (b, int(nseg[b]), S)
        want_seg.append(a64), twin_seg.append(a32), want_score.append(float(sr.score(a64))), twin_score.append(float(sr.score(a32)))
    assert nseg.tolist() == [0, 1, 2, 8, 9] and score[0] == 0.0
    got = np.concatenate([seg[b, :len(a)] for b, a in enumerate(want_seg)])
    w64, w32 = np.concatenate(want_seg), np.concatenate(twin_seg).astype(np.float64)
    dist = float(np.abs(w64 - w32).max())
    tag = 'mode %d %s' % (mode, variant)
    print('MEASURED score %s: largest twin distance %.3e' % (tag, dist))
    _measured('seg ' + tag, got, w64, 4.0 * dist)
    _measured('score ' + tag, score, np.array(want_score), np.where(np.array(want_score) == 0.0, 0.0, 4.0 * dist))
    if variant == 'identical':
        worst = float(np.abs(got.astype(np.float64) - 1.0).max())
        print('MEASURED score %s: largest |seg - 1| %.3e = %.1f ulp' % (tag, worst, worst / 2.0 ** -23))
        assert worst <= 4 * 2.0 ** -23 and np.abs(score[1:].astype(np.float64) - 1.0).max() <= 4 * 2.0 ** -23
    if variant.startswith('zero'):
        assert np.isfinite(got).all() and got.max() < 1.0


# ------------------------------------------------------------------------------------------ SI-SDR
@pytest.mark.parametrize('zero_mean', (1, 0))
def test_si_sdr_against_float64(zero_mean):
    """len in {0, 1, 1023, 1024, 1025} (below, at and above the 1,024 lanes), a reference of zeros, y == x (+inf), and a DC
    offset of 100 amplitudes with the mean removed and kept, y == 0 and a y exactly orthogonal to x (alpha == 0: -inf, valid 1).  The device's sums are float64 and the dB value is rounded to
    float32 once: |error| <= u |dB| plus 1e-9 dB for the float64 sums' own order (relative 1e-12 on the ratio at most at these
    lengths and distortions)."""
    ref, deg, lens, tags = sc.si_sdr_batch()
    rc, s, v = _si_call(ref, deg, lens, zero_mean)
    assert rc == 0 and not np.isnan(s).any()
    for b, tag in enumerate(tags):
        want, valid = sr.si_sdr(np.nan_to_num(ref[b]), np.nan_to_num(deg[b]), lens[b], bool(zero_mean))
        assert int(v[b]) == valid, (tag, int(v[b]), valid)
        if tag == 'len1' and valid:
            # one sample is a multiple of the reference: the residual is 0 or the rounding of alpha x, +inf or beyond 300 dB
            assert want > 300.0 and s[b] > 300.0, (tag, s[b], want)
            continue
        if np.isinf(want) or not valid:
            assert s[b] == np.float32(want), (tag, s[b], want)
            continue
        _measured('si_sdr %s zero_mean=%d (%.3f dB)' % (tag, zero_mean, want), s[b:b + 1], np.array([want]), U * abs(want) + 1e-9)
    assert v.tolist() == [0, 1 - zero_mean, 1, 1, 1, 0, 1, 1, 1, 1] and s[0] == 0.0 and s[5] == 0.0 and s[6] == np.inf
    assert s[8] == -np.inf and s[9] == -np.inf                     # y == 0, and y orthogonal to x: alpha == 0, valid stays 1
    clean_r, clean_d = np.where(np.isnan(ref), 0.5, ref)[2:5, :1023], np.where(np.isnan(deg), -0.25, deg)[2:5, :1023]
    rc, s0, v0 = _si_call(clean_r, clean_d, None, zero_mean)
    rc1, s1, v1 = _si_call(clean_r, clean_d, [1023, 2000, 1023], zero_mean)
    assert rc == 0 and rc1 == 0 and _same_bits(s0, s1) and v0.tolist() == v1.tolist() == [1, 1, 1]
    assert abs(float(s0[0]) - sr.si_sdr(clean_r[0], clean_d[0], None, bool(zero_mean))[0]) <= U * abs(float(s0[0])) + 1e-9


# ------------------------------------------------------------------------------------------ identity
def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype)


def _inputs(k, B=4, L=sc.len_for_frames(45) + 3):
    """Replay k's batch of four pairs: other noise, other lengths (one below 30 frames)."""
    lens = np.array([L - 3 - 11 * k, sc.len_for_frames(33 + k), sc.len_for_frames(12 + k), L - 200 * (k + 1)], np.int32)
    ref, deg = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    for b in range(B):
        ref[b, :lens[b]] = sc.modulated(lens[b], 200 + 10 * k + b)
        deg[b, :lens[b]] = ref[b, :lens[b]] + sc.noise(lens[b], 300 + 10 * k + b, 0.03).astype(np.float32)
    return [_t(ref), _t(deg), _t(lens, torch.int32)]


def _all_launches(ref, deg, lens):
    """Every launch on torch tensors: stoi_batch's chain in both modes with the intermediate results, and SI-SDR."""
    import _vc
    import evaluation
    lib, st = _vc.lib(), _vc.current_stream()
    B, L = ref.shape
    maxF = sr.n_frames(L)
    max_m, max_seg = maxF - 1, maxF - sr.N_SEG
    dev = ref.device
    e, nf = torch.empty((B, maxF), device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    idx, K = torch.empty((B, maxF), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    T = torch.empty((2, B, max_m, NB), device=dev)
    tab = evaluation._stoi_bands_device()
    _vc.check(lib.vc_stoi_energy_f32(_vc.ptr(ref), _vc.ptr(lens), B, L, L, _vc.ptr(e), _vc.ptr(nf), maxF, st))
    _vc.check(lib.vc_stoi_keep_f32(_vc.ptr(e), _vc.ptr(nf), B, maxF, RATIO, _vc.ptr(idx), _vc.ptr(K), st))
    _vc.check(lib.vc_stoi_bands_f32(_vc.ptr(ref), _vc.ptr(deg), B, L, L, _vc.ptr(idx), _vc.ptr(K), maxF, _vc.ptr(tab), NB, _vc.ptr(T),
                                    max_m, st))
    out = [e, nf, idx, K, T]
    for mode in (0, 1):
        seg, s, n = torch.empty((B, max_seg), device=dev), torch.empty((B,), device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        _vc.check(lib.vc_stoi_score_f32(_vc.ptr(T), _vc.ptr(K), B, maxF, max_m, NB, mode, _vc.ptr(seg), max_seg, _vc.ptr(s), _vc.ptr(n), st))
        out += [seg, s, n]
    for zm in (0, 1):
        d, v = torch.empty((B,), device=dev), torch.empty((B,), dtype=torch.uint8, device=dev)
        _vc.check(lib.vc_si_sdr_f32(_vc.ptr(ref), _vc.ptr(deg), _vc.ptr(lens), B, L, L, zm, _vc.ptr(d), _vc.ptr(v), st))
        out += [d, v]
    r = evaluation.stoi_batch(ref, deg, lens, return_segments=True)
    x = evaluation.stoi_batch(ref, deg, lens, extended=True)
    return out + [r.score, r.n_segments, r.n_kept, r.seg, x.score]


NAMES = ('energy n_frames index n_kept T seg0 score0 nseg0 seg1 score1 nseg1 sdr0 valid0 sdr1 valid1 '
         'stoi.score stoi.n_segments stoi.n_kept stoi.seg estoi.score').split()


def test_alone_batch_of_four_graph_replay_and_repeats_agree_bit_for_bit():
    """Every launch and stoi_batch: a repeated call, each utterance alone, and a graph captured on another batch and replayed
    on this one give the bits of the eager batch of four."""
    from test_graph_replay_gpu import _capture, _free, _same
    static = _inputs(0)
    g, outs = _capture(lambda: _all_launches(*static))
    try:
        for k in (1, 2):
            new = _inputs(k)
            for s, t in zip(static, new):
                s.copy_(t)
            g.replay()
            torch.cuda.synchronize()
            want = _all_launches(*new)
            again = _all_launches(*new)
            for name, a, b, c in zip(NAMES, outs, want, again):
                _same(a, b, 'replay %d %s' % (k, name))
                _same(c, b, 'repeat %d %s' % (k, name))
            frames = [sr.n_frames(n) for n in new[2].cpu().tolist()]
            assert want[3].cpu().tolist() == frames and frames[1:3] == [33 + k, 12 + k]
            assert want[7].cpu().tolist() == [max(f - sr.N_SEG, 0) for f in frames] and 0.0 < float(want[6][0]) <= 1.0 and float(want[6][2]) == 0.0
            _same(want[15], want[6], 'stoi_batch is the chain: score')
            _same(want[18], want[5], 'stoi_batch is the chain: seg')
            _same(want[19], want[9], 'stoi_batch is the chain: ESTOI')
            if k == 1:
                ref, deg, lens = new
                for b in range(4):
                    one = _all_launches(ref[b:b + 1].clone(), deg[b:b + 1].clone(), lens[b:b + 1].clone())
                    for name, a, w in zip(NAMES, one, want):
                        w = w[:, b:b + 1] if name == 'T' else w[b:b + 1]
                        _same(a, w, 'alone utt %d %s' % (b, name))
    finally:
        _free(g)


# ------------------------------------------------------------------------------------------ end to end
def test_stoi_batch_is_the_chained_restatement_and_orders_the_noisy_vowel():
    """evaluation.stoi_batch at 10 kHz on the modulated vowel in white noise at 20 / 10 / 0 / -10 dB (one batch, ragged by a
    few samples, numpy in): each score equals the chained float64 restatement within the score bound: 4 x the distance
    between that chain and its float32 twin (band twin, then score twin) on the case, taken for the segments and for the score
    each; and both scores fall strictly with the SNR on the device.  si_sdr_batch gives the restatement's dB."""
    import evaluation
    snrs = (20, 10, 0, -10)
    pairs = [sc.vowel_pair(s) for s in snrs]
    L = len(pairs[0][0])
    lens = [L, L - 1, L - 130, L - 5]
    ref = np.stack([p[0] for p in pairs]).astype(np.float32)
    deg = np.stack([p[1] for p in pairs]).astype(np.float32)
    got = {}
    for ext in (False, True):
        r = evaluation.stoi_batch(ref, deg, lens, extended=ext, return_segments=True)
        got[ext] = r.score.cpu().numpy()
        nseg, nk = r.n_segments.cpu().numpy(), r.n_kept.cpu().numpy()
        for b, snr in enumerate(snrs):
            x, y = pairs[b][0][:lens[b]], pairs[b][1][:lens[b]]
            want, seg, d_seg, d_score = sr.chain_distance(x, y, extended=ext)
            assert int(nk[b]) == len(sr.kept(sr.energies(x))) and int(nseg[b]) == len(seg) == int(nk[b]) - sr.N_SEG
            name = 'ESTOI' if ext else 'STOI'
            print('MEASURED %s vowel at %+d dB: chained twin distance %.3e (segments), %.3e (score)' % (name, snr, d_seg, d_score))
            _measured('%s vowel at %+d dB (%.4f)' % (name, snr, want), got[ext][b:b + 1], np.array([want]), 4.0 * d_score)
            _measured('%s vowel at %+d dB segments' % (name, snr), r.seg[b, :len(seg)].cpu().numpy(), seg, 4.0 * d_seg)
            assert not r.seg[b, len(seg):].any()
        assert (np.diff(got[ext]) < 0).all(), got[ext]
    d = evaluation.si_sdr_batch(ref, deg, lens)
    for b, snr in enumerate(snrs):
        want = sr.si_sdr(pairs[b][0], pairs[b][1], lens[b])[0]
        _measured('SI-SDR vowel at %+d dB (%.3f dB)' % (snr, want), d.si_sdr[b:b + 1].cpu().numpy(), np.array([want]), U * abs(want) + 1e-9)
    assert d.valid.cpu().tolist() == [1, 1, 1, 1]
    print('MEASURED device vowel: STOI %s ESTOI %s' % (np.round(got[False], 4).tolist(), np.round(got[True], 4).tolist()))


def test_stoi_batch_at_16_khz_is_stoi_batch_on_the_resamplers_output():
    """wav_sr=16000: both sides through audio_lib.resample_batch, then the 10 kHz chain on its output and its lengths: bit
    for bit; tensors and host lengths in, None lengths too."""
    import audio_lib
    import evaluation
    rng = np.random.RandomState(8)
    L = 16000
    t = np.arange(L) / 16000.0
    ref = (0.2 * np.sin(2 * np.pi * 440.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)))[None].repeat(2, 0).astype(np.float32)
    ref[1] = 0.1 * rng.standard_normal(L)
    deg = (ref + 0.02 * rng.standard_normal(ref.shape)).astype(np.float32)
    lens = [L, 12345]
    got = evaluation.stoi_batch(_t(ref), _t(deg), lens, wav_sr=16000, return_segments=True)
    r10, l10 = audio_lib.resample_batch(_t(ref), lens, sr_in=16000, sr_out=10000)
    d10, _ = audio_lib.resample_batch(_t(deg), lens, sr_in=16000, sr_out=10000)
    assert l10.tolist() == [10000, 7716]
    want = evaluation.stoi_batch(r10, d10, l10, return_segments=True)
    for name in ('score', 'n_segments', 'n_kept', 'seg'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert int(got.n_segments.min()) > 0 and bool(torch.isfinite(got.score).all())
    full = evaluation.stoi_batch(ref, deg, None, wav_sr=16000)
    assert torch.equal(full.score[:1], got.score[:1]) and full.seg is None
