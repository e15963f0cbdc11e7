"""Host side of the resampler (no GPU): audio_lib.resample_taps against the closed form, the float64 reference of
tests/resample_ref.py against scipy's polyphase resampler run on the same taps, the length contract in exact integers,
the identity at equal rates, every validation error, the ABI of the three new exports, and convert_batch's host
planning on resampled lengths."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import resample_ref as rr
from test_convert_batch_cpu import CFG, _NoDecoder

RATES = [(48000, 16000), (44100, 16000), (22050, 16000), (32000, 16000), (8000, 16000), (11025, 16000), (16000, 48000),
         (16000, 44100)]
PRESETS = ['kaiser_best', 'kaiser_fast']


@pytest.mark.parametrize('res_type', PRESETS)
@pytest.mark.parametrize('sr_in,sr_out', RATES)
def test_taps_are_the_closed_form(sr_in, sr_out, res_type):
    import audio_lib
    up, down, half, g = audio_lib.resample_taps(sr_in, sr_out, res_type)
    gcd = math.gcd(sr_in, sr_out)
    assert (up, down) == (sr_out // gcd, sr_in // gcd)
    Z, rolloff, beta = audio_lib.RES_TYPES[res_type]
    assert audio_lib.RES_TYPES[res_type] == rr.PRESETS[res_type]
    fc = rolloff * min(1.0, up / down)
    assert half == math.ceil(Z * up / fc) - 1
    assert g.dtype == np.float64 and g.shape == (2 * half + 1,)
    assert np.array_equal(g, g[::-1])                                        # symmetric, bit for bit
    for k in (0, 1, up, up + 1, 7 * up, half // 2, half - 1, half, -3, -half):
        want = rr.h_closed(k / up, fc, Z, beta)
        assert abs(g[k + half] - want) <= 1e-15 * fc + 1e-12 * abs(want), (k, g[k + half], want)
    assert abs(g[half] - fc) <= 4e-16 * fc                                  # h(0) = fc
    # the first tap left out is outside the window (or exactly on its edge)
    assert rr.h_closed((half + 1) / up, fc, Z, beta) == 0.0
    assert np.allclose(g, rr.taps(sr_in, sr_out, res_type)[3], rtol=1e-13, atol=1e-300)
    # a (Z, rolloff, beta) tuple is the same thing
    assert np.array_equal(audio_lib.resample_taps(sr_in, sr_out, (Z, rolloff, beta))[3], g)


@pytest.mark.parametrize('res_type', PRESETS)
@pytest.mark.parametrize('sr_in,sr_out', RATES)
def test_dc_gain_of_every_phase(sr_in, sr_out, res_type):
    """Every phase's taps sum to (nearly) the same gain: a constant input comes out constant.  The yardstick is the float64
    reference itself: its output for x = 1, away from the edges, deviates from 1 by what the window's stop band leaks;
    no phase of audio_lib's taps may deviate by more than that run's worst."""
    import audio_lib
    up, down, half, g = audio_lib.resample_taps(sr_in, sr_out, res_type)
    edge = (half // up + 2) * up // down + 3                                # outputs whose taps reach past an end
    n_in = (up + 2 * edge + 4) * down // up + 1
    y = rr.resample(np.ones(n_in), sr_in, sr_out, res_type)
    inner = y[edge:len(y) - edge]
    assert len(inner) >= up                                                  # every phase occurs
    dev_ref = np.abs(inner - 1.0).max()
    sums = np.array([g[(p + half) % up::up].sum() for p in range(up)])       # k = p (mod up)
    print('%d -> %d %s: DC gain %.8f .. %.8f, reference deviation %.3e' % (sr_in, sr_out, res_type, sums.min(), sums.max(), dev_ref))
    assert np.abs(sums - 1.0).max() <= dev_ref + 1e-13
    assert dev_ref < (1e-6 if res_type == 'kaiser_best' else 1e-3)


@pytest.mark.parametrize('res_type', PRESETS)
@pytest.mark.parametrize('sr_in,sr_out', RATES)
def test_float64_reference_is_scipy_resample_poly_on_the_same_taps(sr_in, sr_out, res_type):
    from scipy import signal
    up, down, half, g = rr.taps(sr_in, sr_out, res_type)
    rng = np.random.RandomState(sr_in % 997)
    for n_in in (3 * down + 1, 2000, 4801):
        x = rng.standard_normal(n_in)
        want = signal.resample_poly(x, up, down, window=g / up)             # scipy multiplies the window by `up`
        got = rr.resample(x, sr_in, sr_out, res_type)
        assert got.shape == want.shape == (rr.out_len(n_in, sr_in, sr_out),)
        e = np.abs(got - want).max() / np.abs(want).max()
        print('%d -> %d %s n=%d: |ref - resample_poly| / peak = %.2e' % (sr_in, sr_out, res_type, n_in, e))
        assert e <= 1e-12


def test_resample_len_is_ceil_in_exact_integers():
    import audio_lib
    from fractions import Fraction
    for sr_in, sr_out in RATES + [(44100, 48000), (16000, 16000), (7, 3)]:
        up, down = rr.ratio(sr_in, sr_out)
        for n in [0, 1, 2, down - 1, down, down + 1, 79999, 80000, 80001, 2 ** 31 // up - 1, 2 ** 31 // up, 2 ** 31 // up + 1,
                  2 ** 31 - 1, 2 ** 40 + 1]:
            want = math.ceil(Fraction(n * sr_out, sr_in))
            got = audio_lib.resample_len(n, sr_in, sr_out)
            assert got == want and isinstance(got, int), (sr_in, sr_out, n, got, want)
    a = audio_lib.resample_len(np.array([1, 441, 442, 2 ** 31 - 1]), 44100, 16000)
    assert a.dtype == np.int64 and a.tolist() == [1, 160, 161, math.ceil(Fraction((2 ** 31 - 1) * 160, 441))]
    assert audio_lib.resample_len(np.int32(2 ** 31 - 1), 16000, 48000) == 3 * (2 ** 31 - 1)       # no int32 wrap


def test_equal_rates_return_the_same_object():
    import audio_lib
    y = np.arange(10, dtype=np.float32)
    assert audio_lib.resample(y, 16000, 16000) is y
    assert audio_lib.resample(y, 48000, 48000, 'kaiser_fast') is y
    w = np.zeros((2, 100), np.float32)
    out, lens = audio_lib.resample_batch(w, [100, 60], sr_in=22050, sr_out=22050)
    assert out is w and list(lens) == [100, 60]
    up, down, half, g = audio_lib.resample_taps(16000, 16000)
    assert (up, down) == (1, 1) and half == math.ceil(64 / 0.9475937167399596) - 1


def test_every_validation_error_precedes_gpu_work():
    import audio_lib
    import conversion
    w = np.zeros((2, 1000), np.float32)
    for bad in (0, -16000, 44100.0, '48000', None, True):
        with pytest.raises(ValueError, match=r' - ERROR, resample.*positive integer'):
            audio_lib.resample_taps(bad, 16000)
        with pytest.raises(ValueError, match=r' - ERROR, resample'):
            audio_lib.resample_batch(w, None, sr_in=bad)
        with pytest.raises(ValueError, match=r' - ERROR, resample.*positive integer'):
            audio_lib.resample_len(10, 16000, bad)
        with pytest.raises(ValueError, match=r' - ERROR, resample.*positive integer'):
            audio_lib.resample(w[0], bad, 16000)
    for bad in ('kaiser_slow', 'sinc', (64, 0.9), (0, 0.9, 8.0), (64, 1.5, 8.0), (64, 0.9, float('nan')), 5):
        with pytest.raises(ValueError, match=r' - ERROR, resample.*res_type'):
            audio_lib.resample_taps(48000, 16000, bad)
        with pytest.raises(ValueError, match=r' - ERROR, resample.*res_type'):
            audio_lib.resample_batch(w, None, sr_in=48000, res_type=bad)
        with pytest.raises(ValueError, match=r' - ERROR, resample.*res_type'):
            conversion.convert_batch(_NoDecoder(), np.zeros((1, 240000), np.float32), cfg_d=CFG, wav_sr=48000, res_type=bad)
    for bad in ([1000], [1000, 1001], [0, 1000], [-5, 10], [[1000, 1000]] * 2):
        with pytest.raises(ValueError, match=r' - ERROR, resample_batch: lens'):
            audio_lib.resample_batch(w, bad, sr_in=48000)
    with pytest.raises(ValueError, match=r' - ERROR, resample_batch: wav'):
        audio_lib.resample_batch(w[0], None, sr_in=48000)
    # convert_batch: rates, lens at wav_sr, and the front-end's own limit on the RESAMPLED length
    wav = np.zeros((3, 240000), np.float32)                                  # 5 s at 48 kHz
    for bad in (0, -1, 44100.5, '48000'):
        with pytest.raises(ValueError, match=r'positive integer'):
            conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, wav_sr=bad)
        with pytest.raises(ValueError, match=r'positive integer'):
            conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, out_sr=bad)
    with pytest.raises(ValueError, match=r'lens'):
        conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[240000, 240001, 1000], wav_sr=48000)
    with pytest.raises(ValueError, match=r'lens'):
        conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[240000, 0, 1000], wav_sr=48000)
    with pytest.raises(ValueError, match=r'n_fft//2'):                       # 600 samples at 48 kHz are 200 at 16 kHz
        conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[240000, 600, 240000], wav_sr=48000)
    conversion.convert_plan([audio_lib.resample_len(603, 48000, 16000)], CFG)       # ... and 201 would do
    # a valid call reaches the device check
    import _vc
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            audio_lib.resample_batch(w, [1000, 500], sr_in=48000)
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            audio_lib.resample(w[0], 44100, 16000)
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[240000, 120000, 200000], wav_sr=48000, out_sr=44100)


def test_new_exports_are_declared_exported_and_bound():
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    assert int(re.search(r'#define\s+VC_ABI_VERSION\s+(\d+)', hdr).group(1)) == 7 == _vc.VC_ABI_VERSION
    lib = _vc.lib()
    assert lib.vc_version() == 7
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, ret in (('vc_resample_plan_create', 'int'), ('vc_resample_plan_destroy', 'void'), ('vc_resample_f32', 'int')):
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), code), name
        assert name in _vc._SIGS and hasattr(lib, name)
    assert 'double' not in ''.join(re.findall(r'vc_resample_\w+\s*\(([^)]*)\)', code)).replace('const double*', '')
    # validation precedes any HIP call (no GPU needed)
    g = np.ones(5)
    h = ctypes.c_void_p()
    assert lib.vc_resample_plan_create(1, 3, 2, None, ctypes.byref(h)) == 1 and b'vc_resample_plan_create' in lib.vc_last_error()
    assert lib.vc_resample_plan_create(1, 3, 2, _vc.ptr(g), None) == 1
    assert lib.vc_resample_plan_create(0, 3, 2, _vc.ptr(g), ctypes.byref(h)) == 1
    assert lib.vc_resample_plan_create(1, -3, 2, _vc.ptr(g), ctypes.byref(h)) == 1
    assert lib.vc_resample_plan_create(1, 3, -1, _vc.ptr(g), ctypes.byref(h)) == 1 and b'half' in lib.vc_last_error()
    # a ratio whose tile cannot fit the kernel's LDS budget is refused before anything is allocated: VC_ERR_UNSUPPORTED
    assert lib.vc_resample_plan_create(1, 6000, 2, _vc.ptr(g), ctypes.byref(h)) == 4 and b'vc_resample_plan_create' in lib.vc_last_error()
    assert not h.value
    p = ctypes.c_void_p(4096)
    assert lib.vc_resample_f32(None, p, None, 1, 100, 100, p, 34, 34, None) == 1 and b'vc_resample_f32' in lib.vc_last_error()
    lib.vc_resample_plan_destroy(None)                                       # NULL is a no-op


def test_resample_f32_rejects_bad_shapes_without_a_gpu():
    """Shape checks of vc_resample_f32 need a plan, and a plan needs device memory; the checks that do not depend on the
    plan (NULL pointers, batch, strides) are reached with a non-NULL placeholder only where they precede every use of it.
    Those that read up / down are exercised on the GPU (tests/test_resample_gpu.py)."""
    import _vc
    lib = _vc.lib()
    p = ctypes.c_void_p(4096)
    assert lib.vc_resample_f32(p, None, None, 1, 100, 100, p, 34, 34, None) == 1
    assert lib.vc_resample_f32(p, p, None, 1, 100, 100, None, 34, 34, None) == 1
    for batch, max_in, ld_in, max_out, ld_out in ((0, 100, 100, 34, 34), (-1, 100, 100, 34, 34), (1, 0, 100, 34, 34),
                                                  (1, 100, 99, 34, 34), (1, 100, 100, 0, 34), (1, 100, 100, 34, 33),
                                                  (70000, 100, 100, 34, 34)):
        assert lib.vc_resample_f32(p, p, None, batch, max_in, ld_in, p, max_out, ld_out, None) == 1, (batch, max_in, ld_in, max_out, ld_out)
        assert b'vc_resample_f32: bad shape' in lib.vc_last_error()


def test_a_library_without_the_new_exports_is_refused_with_a_clear_error(tmp_path):
    """The exports were added without a version bump: a stale build that still reports version 7 but lacks them must
    fail at load time with a VCError that names the symbol (a separate interpreter: the binding caches its handle)."""
    import subprocess
    import sys
    src = tmp_path / 'stale.c'
    src.write_text('int vc_version(void) { return 7; }\n')
    so = tmp_path / 'libvc_stale.so'
    subprocess.check_call(['gcc', '-shared', '-fPIC', str(src), '-o', str(so)])
    code = ('import sys; sys.path.insert(0, %r); import _vc\n'
            'try:\n    _vc.lib()\nexcept _vc.VCError as e:\n    print("REFUSED", e)\n' % os.path.join(ROOT, 'speech-cloner_amd'))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, VC_LIB_PATH=str(so)), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'REFUSED' in r.stdout and 'does not export' in r.stdout, r.stdout + r.stderr


def test_convert_batch_plans_on_resampled_lengths(monkeypatch):
    """convert_batch(wav_sr=48000) hands convert_plan the lengths at 16 kHz: ceil(len / 3)."""
    import audio_lib
    import conversion
    seen = []
    real = conversion.convert_plan

    def spy(lens, *a, **kw):
        seen.append([int(v) for v in lens])
        return real(lens, *a, **kw)

    monkeypatch.setattr(conversion, 'convert_plan', spy)
    wav = np.zeros((3, 240000), np.float32)
    lens48 = [240000, 120001, 76802]
    try:
        conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=lens48, wav_sr=48000, phase=np.zeros((1, 1, 1)))
    except ValueError as e:                                                  # stops at the phase shape check, after the plan
        assert 'phase' in str(e)
    assert seen == [[80000, 40001, 25601]]
    assert seen[0] == [audio_lib.resample_len(n, 48000, 16000) for n in lens48]
    plan = real(seen[0], CFG, 0, 60, True)
    assert list(plan.n_src) == [1001, 501, 321] and list(plan.N) == [3, 2, 1]
    # wav_sr equal to the configuration's rate, or None: the lengths as given
    for sr in (None, 16000):
        seen.clear()
        try:
            conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=lens48, wav_sr=sr, phase=np.zeros((1, 1, 1)))
        except ValueError as e:
            assert 'phase' in str(e)
        assert seen == [lens48]
