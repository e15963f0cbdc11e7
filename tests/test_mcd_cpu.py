"""Host side of evaluation.py (no GPU): the float64 reference of tests/mcd_ref.py against a plain double loop (ties
included), the DCT table against scipy, the dB scale against the textbook formula, the band rule, every validation
error, and the ABI of the five new exports."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import mcd_ref as mr

CFG = {'sample_rate': 16000, 'pre_emphasis': 0.97, 'hop_length': 80, 'win_length': 400, 'n_fft': 400, 'n_mels': 80, 'n_mfcc': 40,
       'window': 'hann', 'mfcc_normaleze_first_mfcc': True, 'mfcc_norm_factor': 0.01, 'calc_mfcc_derivate': True,
       'M_dB_norm_factor': 0.01, 'P_dB_norm_factor': 0.01, 'mean_abs_amp_norm': 0.003, 'clip_output': True, 'n_timesteps': 400}


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1], (a[:2], b[:2])
    if a[2] is None or b[2] is None:
        assert a[2] is None and b[2] is None
    else:
        assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize('Fa,Fb', [(1, 1), (1, 7), (9, 1), (5, 5), (12, 17), (23, 11), (40, 37)])
@pytest.mark.parametrize('band', [None, 0, 2, 50])
def test_antidiagonal_reference_equals_the_double_loop(Fa, Fb, band):
    rng = np.random.RandomState(Fa * 100 + Fb)
    ca, cb = rng.standard_normal((Fa, 6)), rng.standard_normal((Fb, 6))
    got, want = mr.dtw(ca, cb, 25.0, band), mr.dtw_loop(ca, cb, 25.0, band)
    _same(got, want)
    if got[2] is not None:
        mr.check_path(got[2], Fa, Fb, band)
        assert len(got[2]) == got[1]
        assert abs(mr.path_cost(ca, cb, got[2], 25.0) - got[0]) <= 1e-12 * got[0]
    # integer-valued frames whose components are all equal: d = 4 |delta| exactly, so ties are everywhere
    ia, ib = rng.randint(0, 3, (Fa, 1)) * np.ones((1, 8)), rng.randint(0, 3, (Fb, 1)) * np.ones((1, 8))
    for dt in (np.float64, np.float32):
        got, want = mr.dtw(ia, ib, 1.0, band, dt), mr.dtw_loop(ia, ib, 1.0, band, dt)
        _same(got, want)
        assert not np.isfinite(got[0]) or got[0] == int(got[0])
    _same(mr.dtw(ia, ib, 1.0, band, np.float32), mr.dtw(ia, ib, 1.0, band, np.float64))


def test_known_small_cases():
    a = np.arange(6, dtype=np.float64)[:, None] * np.ones((1, 8))
    total, n, path = mr.dtw(a, a)
    assert total == 0 and n == 6 and np.array_equal(path, np.stack([np.arange(6)] * 2, 1))       # ties take the diagonal
    b = np.repeat(a, 3, axis=0)
    total, n, path = mr.dtw(a, b)
    assert total == 0 and n == 18 and np.array_equal(path[:, 1], np.arange(18))
    total, n, path = mr.dtw(a[:1], a[:4])
    assert (total, n) == (4.0 * (1 + 2 + 3), 4) and np.array_equal(path, [[0, 0], [0, 1], [0, 2], [0, 3]])
    assert mr.frame_mcd(a, a[::-1]) == 4.0 * (5 + 3 + 1 + 1 + 3 + 5) / 6


def test_dct_table_is_scipys_orthonormal_dct2():
    from scipy import fft
    import evaluation
    for n_mels, n_coef, first in ((80, 24, 1), (80, 13, 0), (128, 32, 1), (40, 40 - 8, 8)):
        want = fft.dct(np.eye(n_mels), type=2, norm='ortho', axis=0)[first:first + n_coef]
        t = mr.dct_table(n_mels, n_coef, first)
        # the cosine's argument reaches pi * 40 and is rounded three times on the way: 0.16 * 126 * 3 * 2^-52
        assert np.abs(t - want).max() <= 2e-14
        got = evaluation.dct_rows(n_mels, n_coef, first)
        assert got.dtype == np.float32 and got.shape == (n_coef, n_mels)
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24          # one rounding of values below 1/2 ... 2^-25; a margin of 2
        x = np.random.RandomState(0).standard_normal((5, n_mels))
        assert np.allclose(mr.cepstra(x, n_coef, first), fft.dct(x, type=2, norm='ortho', axis=-1)[:, first:first + n_coef], atol=1e-13)


def test_default_scale_is_the_textbook_decibel_formula():
    """Two mel tensors built the way the front-end builds them from known log-amplitude spectra (reference
    audio_lib.py:172, 234-235: M_dB_norm_factor * (20 log10(mel power) - min)); the distance with scale 1 / (4 M) must be
    (10 / ln 10) * sqrt(2 sum_d (mc_a - mc_b)^2) on cepstra of the natural log amplitude.  Gain and the minimum move c0
    only."""
    rng = np.random.RandomState(4)
    for M in (0.01, 0.0125, 0.02):
        ln_a, ln_b = rng.standard_normal((30, 80)), rng.standard_normal((30, 80))
        mels = []
        for ln_amp, gain in ((ln_a, 1.0), (ln_b, 0.37)):
            power = (gain * np.exp(ln_amp)) ** 2
            db = 20.0 * np.log10(power)
            mels.append(M * (db - db.min()))
        got = mr.dist(mr.cepstra(mels[0]), mr.cepstra(mels[1]), mr.default_scale(M))
        mc_a, mc_b = mr.cepstra(ln_a), mr.cepstra(ln_b)
        want = 10.0 / math.log(10.0) * np.sqrt(2.0 * ((mc_a - mc_b) ** 2).sum(-1))
        assert np.abs(got - want).max() <= 1e-11 * want.max()
    assert mr.default_scale(0.01) == 25.0


def test_band_rule():
    for Fa, Fb in ((1, 1), (1, 9), (9, 1), (10, 10), (100, 137), (3000, 3700), (16384, 1), (16384, 16384)):
        for w in (0, 1, 5, 10 ** 6):
            assert mr.allowed(Fa - 1, Fb - 1, Fa, Fb, w) and mr.allowed(0, 0, Fa, Fb, w)
        if Fa * Fb <= 20000:
            i, j = np.meshgrid(np.arange(Fa), np.arange(Fb), indexing='ij')
            for w in (0, 1, 3, 20):
                m = mr.allowed(i, j, Fa, Fb, w)
                assert np.array_equal(m, mr.allowed(j, i, Fb, Fa, w))        # a <-> b: cell (j, i) of the swapped pair
                if w >= 1:                                                     # a stripe one frame wide holds a connected staircase
                    assert np.isfinite(mr.dtw(np.zeros((Fa, 1)), np.zeros((Fb, 1)), 1.0, w, want_path=False)[0])
            assert mr.allowed(i, j, Fa, Fb, None).all()
    # swapping a and b transposes the path and keeps the score
    rng = np.random.RandomState(1)
    ca, cb = rng.standard_normal((31, 4)), rng.standard_normal((47, 4))
    for w in (None, 2, 6):
        t1, n1, p1 = mr.dtw(ca, cb, 1.0, w)
        t2, n2, p2 = mr.dtw(cb, ca, 1.0, w)
        assert abs(t1 - t2) <= 1e-12 * t1


def test_every_validation_error_precedes_gpu_work():
    import evaluation as ev
    mel = np.zeros((2, 50, 80), np.float32)
    for bad in (np.zeros((50, 80), np.float32), np.zeros((2, 0, 80), np.float32), 5):
        with pytest.raises(ValueError, match=r' - ERROR, .*\[B, F, n_mels\]'):
            ev.mel_cepstra(bad)
        with pytest.raises(ValueError, match=r' - ERROR, mcd_batch: mel_a'):
            ev.mcd_batch(bad, mel, [50, 50], [50, 50], CFG)
    with pytest.raises(ValueError, match=r'agree in B and n_mels'):
        ev.mcd_batch(mel, np.zeros((2, 50, 64), np.float32), [50, 50], [50, 50], CFG)
    with pytest.raises(ValueError, match=r'agree in B and n_mels'):
        ev.mcd_batch(mel, np.zeros((3, 50, 80), np.float32), [50, 50], [50, 50, 50], CFG)
    for n_coef, first in ((80, 1), (24, 57), (0, 1), (24, -1)):
        with pytest.raises(ValueError, match=r'n_coef \+ first_coef <= n_mels'):
            ev.mel_cepstra(mel, n_coef, first)
        with pytest.raises(ValueError, match=r'n_coef \+ first_coef <= n_mels'):
            ev.mcd_batch(mel, mel, [50, 50], [50, 50], CFG, n_coef=n_coef, first_coef=first)
    with pytest.raises(ValueError, match=r'at most 32 coefficients'):
        ev.mel_cepstra(mel, 40, 1)
    for bad in ([50], [50, 51], [0, 50], [-1, 3], [50.0, 50.0], [[50, 50]]):
        with pytest.raises(ValueError, match=r'len_a must be 2 integers in \[1, 50\]'):
            ev.mcd_batch(mel, mel, bad, [50, 50], CFG)
        with pytest.raises(ValueError, match=r'len_b must be 2 integers in \[1, 50\]'):
            ev.dtw_batch(mel, mel, [50, 50], bad)
    for bad in ('DTW', 'linear', None, 0):
        with pytest.raises(ValueError, match=r"align must be 'dtw' or 'frame'"):
            ev.mcd_batch(mel, mel, [50, 50], [50, 50], CFG, align=bad)
    for bad in (-1, -100, 2.5, '3', True):
        with pytest.raises(ValueError, match=r'band must be None or a non-negative integer'):
            ev.mcd_batch(mel, mel, [50, 50], [50, 50], CFG, band=bad)
        with pytest.raises(ValueError, match=r'band must be None or a non-negative integer'):
            ev.dtw_batch(mel, mel, [50, 50], [50, 50], band=bad)
    with pytest.raises(ValueError, match=r'pass cfg_d .* or scale'):
        ev.mcd_batch(mel, mel, [50, 50], [50, 50])
    for bad in (0.0, -25.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match=r'scale must be finite and positive'):
            ev.mcd_batch(mel, mel, [50, 50], [50, 50], scale=bad)
    with pytest.raises(ValueError, match=r'agree in B and n_coef'):
        ev.dtw_batch(np.zeros((2, 5, 24), np.float32), np.zeros((2, 5, 12), np.float32), [5, 5], [5, 5])
    with pytest.raises(ValueError, match=r'must be \[B, F, n_coef\]'):
        ev.dtw_batch(np.zeros((5, 24), np.float32), np.zeros((2, 5, 24), np.float32), [5, 5], [5, 5])
    big = np.broadcast_to(np.zeros((1, 1, 24), np.float32), (1, 16385, 24))
    with pytest.raises(ValueError, match=r'at most 16384 frames'):
        ev.dtw_batch(big, big, [10], [10])
    many = np.broadcast_to(np.zeros((1, 1, 24), np.float32), (33, 16384, 24))      # 2^26 bytes per pair
    with pytest.raises(ValueError, match=r'more than 2 GiB of predecessor codes'):
        ev.dtw_batch(many, many, [10] * 33, [10] * 33, return_path=True)
    # the waveform form: shapes, lengths at the side's own rate, the front-end's limit on the resampled length, rates
    wav = np.zeros((2, 48000), np.float32)
    with pytest.raises(ValueError, match=r'cfg_d .* is required'):
        ev.mcd_wav_batch(wav, None, wav, None, None)
    with pytest.raises(ValueError, match=r'wav_b must be \[B, Lmax\]'):
        ev.mcd_wav_batch(wav, None, wav[0], None, CFG)
    with pytest.raises(ValueError, match=r'lens of wav_a'):
        ev.mcd_wav_batch(wav, [48000, 48001], wav, None, CFG)
    with pytest.raises(ValueError, match=r'wav_b needs more than n_fft//2 = 200'):
        ev.mcd_wav_batch(wav, None, wav, [48000, 600], CFG, wav_sr_b=48000)
    with pytest.raises(ValueError, match=r'positive integer'):
        ev.mcd_wav_batch(wav, None, wav, None, CFG, wav_sr_a=44100.5)
    with pytest.raises(ValueError, match=r'res_type'):
        ev.mcd_wav_batch(wav, None, wav, None, CFG, wav_sr_a=48000, res_type='sinc')
    with pytest.raises(ValueError, match=r'same number of utterances'):
        ev.mcd_wav_batch(wav, None, wav[:1], None, CFG)
    with pytest.raises(ValueError, match=r"align must be 'dtw' or 'frame'"):
        ev.mcd_wav_batch(wav, None, wav, None, CFG, align='x')
    # a valid call reaches the device check
    import _vc
    import torch
    if not torch.cuda.is_available():
        for call in (lambda: ev.mel_cepstra(mel), lambda: ev.dtw_batch(mel[:, :, :24], mel[:, :, :24], [50, 3], [1, 50], band=3),
                     lambda: ev.mcd_batch(mel, mel, [50, 3], [1, 50], CFG, return_path=True),
                     lambda: ev.mcd_batch(mel, mel, [50, 3], [1, 50], scale=25.0, align='frame'),
                     lambda: ev.mcd_wav_batch(wav, [48000, 700], wav, None, CFG, wav_sr_a=48000)):
            with pytest.raises(_vc.VCError, match='needs a GPU'):
                call()


def test_new_exports_are_declared_exported_and_bound():
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    assert int(re.search(r'#define\s+VC_ABI_VERSION\s+(\d+)', hdr).group(1)) == 7 == _vc.VC_ABI_VERSION
    lib = _vc.lib()
    assert lib.vc_version() == 7
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, ret in (('vc_mel_cepstra', 'int'), ('vc_dtw_workspace_size', 'size_t'), ('vc_dtw_f32', 'int'),
                      ('vc_dtw_backtrack', 'int'), ('vc_frame_mcd_f32', 'int')):
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), code), name
        assert name in _vc._SIGS and hasattr(lib, name)
    assert 'Evaluation' in hdr


def test_entry_points_refuse_impossible_sizes_before_any_hip_call():
    """No GPU here: a refusal that came after a HIP call would report VC_ERR_HIP (2), not INVALID (1) / UNSUPPORTED (4)."""
    import _vc
    lib = _vc.lib()
    p = ctypes.c_void_p(4096)
    ws = lib.vc_dtw_workspace_size
    assert ws(1, 1001, 1100, 0) == (2 * 1100 * 8 + 255) // 256 * 256                      # O(Fb) per pair
    assert ws(16, 1001, 1100, 0) == 16 * 2 * 1100 * 8
    assert ws(1, 12000, 12000, 0) == 192000                                                # not 576 MB
    assert ws(1, 12000, 12000, 1) == 192000 + 12000 * 750 * 4                              # two bits per cell: 36 MB
    assert ws(1, 16384, 16384, 1) == 2 * 16384 * 8 + 2 ** 26
    for bad in ((0, 10, 10, 0), (1, 0, 10, 0), (1, 10, 0, 0), (1, 16385, 10, 0), (1, 10, 16385, 1), (70000, 10, 10, 0), (-1, 10, 10, 0),
                (64, 16384, 16384, 1)):
        assert ws(*bad) == 0, bad
    assert ws(32, 16384, 16384, 1) > 0 and ws(33, 16384, 16384, 1) == 0

    def dtw(batch=1, max_a=10, max_b=10, n_coef=24, scale=25.0, band=-1, path=0, ca=p, wsb=1 << 40):
        return lib.vc_dtw_f32(ca, p, p, p, batch, max_a, max_b, n_coef, scale, band, path, p, p, p, p, wsb, None)

    assert dtw(ca=None) == 1 and b'vc_dtw_f32: NULL' in lib.vc_last_error()
    for kw in (dict(batch=0), dict(max_a=0), dict(max_b=16385), dict(max_a=-3), dict(batch=65536)):
        assert dtw(**kw) == 1 and b'vc_dtw_f32: bad shape' in lib.vc_last_error(), kw
    for kw in (dict(n_coef=0), dict(scale=0.0), dict(scale=float('nan')), dict(scale=float('inf')), dict(band=-2)):
        assert dtw(**kw) == 1 and b'vc_dtw_f32: need' in lib.vc_last_error(), kw
    assert dtw(n_coef=33) == 4 and b'n_coef 33' in lib.vc_last_error()                     # VC_ERR_UNSUPPORTED
    assert dtw(batch=33, max_a=16384, max_b=16384, path=1) == 4 and b'predecessor codes' in lib.vc_last_error()
    assert dtw(wsb=100) == 3 and b'workspace' in lib.vc_last_error()                       # VC_ERR_WORKSPACE
    bt = lambda batch=1, max_a=10, max_b=10, wsb=1 << 40, w=p: lib.vc_dtw_backtrack(w, wsb, p, p, p, p, batch, max_a, max_b, p, None)
    assert bt(w=None) == 1 and bt(batch=0) == 1 and bt(max_b=16385) == 1 and b'vc_dtw_backtrack' in lib.vc_last_error()
    assert bt(batch=33, max_a=16384, max_b=16384) == 4 and bt(wsb=16) == 3
    fm = lambda batch=1, max_a=10, n_coef=24, scale=25.0, a=p: lib.vc_frame_mcd_f32(a, p, p, p, batch, max_a, 10, n_coef, scale, p, None)
    assert fm(a=None) == 1 and fm(batch=0) == 1 and fm(max_a=0) == 1 and fm(n_coef=0) == 1 and fm(scale=-1.0) == 1
    assert b'vc_frame_mcd_f32' in lib.vc_last_error()
    mc = lambda rows=10, n_mels=80, n_coef=24, dt=0, m=p: lib.vc_mel_cepstra(m, dt, rows, n_mels, p, n_coef, p, None)
    assert mc(m=None) == 1 and mc(rows=0) == 1 and mc(n_coef=81) == 1 and mc(n_coef=33) == 1 and mc(n_mels=513) == 1 and mc(dt=2) == 1
    assert b'vc_mel_cepstra' in lib.vc_last_error()


def test_a_library_without_the_new_exports_is_refused(tmp_path):
    """A build that reports version 7 and has the resampler but not the evaluation exports fails at load time with a
    VCError that names the first missing symbol (a separate interpreter: the binding caches its handle)."""
    import subprocess
    import sys
    import _vc
    have = [n for n in _vc._SIGS if not (n.startswith('vc_dtw') or n in ('vc_mel_cepstra', 'vc_frame_mcd_f32', 'vc_version'))]
    src = tmp_path / 'stale.c'
    src.write_text('int vc_version(void) { return 7; }\n' + ''.join('int %s(void) { return 1; }\n' % n for n in have))
    so = tmp_path / 'libvc_stale.so'
    subprocess.check_call(['gcc', '-shared', '-fPIC', str(src), '-o', str(so)])
    code = ('import sys; sys.path.insert(0, %r); import _vc\n'
            'try:\n    _vc.lib()\nexcept _vc.VCError as e:\n    print("REFUSED", e)\n' % os.path.join(ROOT, 'speech-cloner_amd'))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, VC_LIB_PATH=str(so)), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'REFUSED' in r.stdout and 'does not export vc_mel_cepstra' in r.stdout, r.stdout + r.stderr
