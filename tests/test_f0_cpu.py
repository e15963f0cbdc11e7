"""Host side of the pitch tracker (no GPU): the float64 definition of tests/f0_ref.py on signals of known fundamental,
its invariants (silence, gain, frame count), the float64 figures on built cases, every validation error, and the ABI of
the two new exports."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import f0_ref as fr
from test_mcd_cpu import CFG

SEEDS = (11, 12, 13, 14)


def _track_error(seed):
    x, f0_true, voiced = fr.glide_signal(seed)
    f0, ap = fr.yin(x)
    tau_min, tau_max = fr.lag_range(16000)
    full = fr.fully_voiced_frames(voiced, 80, 512, tau_max)
    centre = np.minimum(np.arange(len(f0)) * 80, len(x) - 1)
    assert full.sum() > 100 and (f0[full] > 0).all(), (seed, full.sum(), (f0[full] == 0).sum())
    return np.abs(fr.cents(f0[full], f0_true[centre][full])), f0, ap, voiced


def test_the_reference_tracks_a_gliding_fundamental():
    """Fully voiced frames of the four 2 s test signals (five harmonics of a fundamental that glides over +- 0.35 octave,
    amplitude modulation, noise of sigma 0.02) against the instantaneous fundamental at the frame's centre.

    Bound, derived: the glide's steepest slope is 0.35 * 2 pi * 1.5 = 3.3 octaves/s; a frame spans at most
    (512 + 267) / 16000 = 49 ms, so F0 moves up to 0.16 octave = 190 cents inside it, and an estimate that averages over
    the span is within half of that of the centre's value: 100 cents.  Measured with these seeds: at most 27.5 cents
    (medians 3.9 to 11.9; 259 fully voiced frames per signal).  A constant five-harmonic tone is tracked far tighter:
    measured 0.034, 0.080 and 0.140 cents at 100, 155.5 and 220 Hz (what the parabola through three samples of d' leaves);
    asserted with a margin of 2: 0.28 cents."""
    worst = 0.0
    for seed in SEEDS:
        e, f0, ap, voiced = _track_error(seed)
        print('seed %d: %d fully voiced frames, median %.2f cents, max %.2f cents' % (seed, len(e), np.median(e), e.max()))
        worst = max(worst, e.max())
        # silence and noise: the frames whose whole span is unvoiced are unvoiced
        tau_max = fr.lag_range(16000)[1]
        none = fr.fully_voiced_frames(~voiced, 80, 512, tau_max)
        assert none.sum() == 0 or (f0[none] == 0).all()
    assert worst <= 100.0
    n = 8000
    tone_worst = 0.0
    for hz in (100.0, 155.5, 220.0):
        x = (0.3 * fr.harmonic_tone(np.full(n, hz))).astype(np.float32)
        f0, ap = fr.yin(x)
        inside = fr.fully_voiced_frames(np.ones(n, bool), 80, 512, 267)
        e = np.abs(fr.cents(f0[inside], hz)).max()
        print('constant %.1f Hz: max %.4f cents, aperiodicity at most %.2e' % (hz, e, ap[inside].max()))
        tone_worst = max(tone_worst, e)
        assert (f0[inside] > 0).all() and ap[inside].max() < 1e-3
    assert tone_worst <= 0.28


def test_silence_gain_and_frame_count():
    for n in (1, 79, 80, 81, 400, 1000):
        f0, ap = fr.yin(np.zeros(n, np.float32))
        assert len(f0) == 1 + n // 80 == fr.n_frames(n, 80)
        assert (f0 == 0).all() and (ap == 1).all()
        for dt in (np.float64, np.float32):
            f0, ap = fr.yin(np.ones(n, np.float32), dtype=dt)
            assert len(f0) == 1 + n // 80 and f0.dtype == dt
    assert len(fr.yin(np.zeros(1000, np.float32), hop=256)[0]) == 1 + 1000 // 256
    x = fr.glide_signal(11, seconds=0.5)[0]
    for dt in (np.float64, np.float32):
        f0, ap = fr.yin(x, dtype=dt)
        assert (f0 > 0).sum() > 20
        for g in (0.5, 4.0, 2.0 ** -20):
            f0g, apg = fr.yin(g * x, dtype=dt)
            assert np.array_equal(f0, f0g) and np.array_equal(ap, apg), (dt, g)


def test_the_float32_restatement_agrees_with_the_definition():
    """The issue's measurement, repeated: on the test signals the two precisions agree on voicing in every frame that is
    not marginal, no more than 1 % are marginal, and F0 / aperiodicity differ by rounding only (the bound here is loose
    on purpose: 1e-3 cents and 1e-4; the device test compares the device against these errors)."""
    x = fr.glide_signal(12, seconds=1.0)[0]
    f64, a64, det = fr.yin(x, details=True)
    f32, a32 = fr.yin(x, dtype=np.float32)
    keep = ~det['marginal']
    assert det['marginal'].mean() <= 0.01
    assert np.array_equal(f64[keep] > 0, f32[keep] > 0)
    both = keep & (f64 > 0)
    e_c, e_a = np.abs(fr.cents(f32[both], f64[both])).max(), np.abs(a32.astype(np.float64) - a64).max()
    print('float32 restatement: %.3e cents, aperiodicity %.3e' % (e_c, e_a))
    assert e_c <= 1e-3 and e_a <= 1e-4
    # the scan of the restatement is a running sum
    d = np.random.RandomState(0).uniform(0, 1, (3, 269)).astype(np.float32)
    assert np.allclose(fr.running_sum(d, np.float32), np.cumsum(d.astype(np.float64), axis=1), rtol=1e-6)


def test_metrics_reference_on_built_cases():
    fa = np.array([100.0, 110.0, 0.0, 150.0, 0.0, 200.0, 220.0])
    m = fr.metrics(fa, fa * 2.0 ** (1.0 / 12.0), 7, 7)
    assert (m['n_cells'], m['n_both_voiced'], m['n_vuv_mismatch']) == (7, 5, 0) and m['vuv_error'] == 0
    assert abs(m['f0_rmse_cents'] - 100.0) <= 1e-10 and abs(m['logf0_corr'] - 1.0) <= 1e-12
    want_hz = np.sqrt(np.mean((fa[fa > 0] * (2.0 ** (1.0 / 12.0) - 1.0)) ** 2))
    assert abs(m['f0_rmse_hz'] - want_hz) <= 1e-10
    # a hand-written path: (i, j) cells, voicing a = V V U V U V V, b = U V V V V U
    fb = np.array([0.0, 115.0, 120.0, 140.0, 180.0, 0.0])
    path = [[0, 0], [1, 1], [2, 1], [2, 2], [3, 3], [4, 3], [4, 4], [5, 4], [6, 5]]
    m = fr.metrics(fa, fb, 7, 6, path)
    #            V/U     V/V     U/V     U/V     V/V     U/V     U/V     V/V     V/U
    assert (m['n_cells'], m['n_both_voiced'], m['n_vuv_mismatch']) == (9, 3, 6) and m['vuv_error'] == 6.0 / 9.0
    c = 1200.0 * np.log2(np.array([110.0 / 115.0, 150.0 / 140.0, 200.0 / 180.0]))
    assert abs(m['f0_rmse_cents'] - np.sqrt((c * c).mean())) <= 1e-10
    assert abs(m['logf0_corr'] - np.corrcoef(np.log2([110.0, 150.0, 200.0]), np.log2([115.0, 140.0, 180.0]))[0, 1]) <= 1e-12
    # cells outside the lengths (the -1 rows beyond a path's end) are skipped and not counted
    assert fr.metrics(fa, fb, 7, 6, path + [[-1, -1], [7, 0], [0, 6]]) == m
    assert fr.metrics(fa, fb, 3, 2, path)['n_cells'] == 3
    # no path: the first min(len_a, len_b) frames
    m = fr.metrics(fa, fb, 7, 6)
    assert (m['n_cells'], m['n_both_voiced'], m['n_vuv_mismatch']) == (6, 2, 4)
    # NaN where undefined
    m = fr.metrics(fa, np.zeros(7), 7, 7)
    assert m['n_both_voiced'] == 0 and m['n_vuv_mismatch'] == 5
    assert np.isnan(m['f0_rmse_cents']) and np.isnan(m['f0_rmse_hz']) and np.isnan(m['logf0_corr'])
    m = fr.metrics(fa, fb, 7, 6, [[1, 1]])
    assert m['n_both_voiced'] == 1 and np.isfinite(m['f0_rmse_cents']) and np.isnan(m['logf0_corr'])       # fewer than 2
    m = fr.metrics(fa, np.full(7, 123.0), 7, 7)
    assert m['n_both_voiced'] == 5 and np.isfinite(m['f0_rmse_hz']) and np.isnan(m['logf0_corr'])           # zero variance
    m = fr.metrics(fa, fb, 7, 6, np.zeros((0, 2), np.int64))
    assert m['n_cells'] == 0 and np.isnan(m['vuv_error'])
    m32 = fr.metrics(fa, fb, 7, 6, path, dtype=np.float32)
    assert m32['n_vuv_mismatch'] == 6 and m32['f0_rmse_cents'].dtype == np.float32


def test_every_validation_error_precedes_gpu_work():
    import evaluation as ev
    wav = np.zeros((2, 4000), np.float32)
    for bad in (np.zeros(4000, np.float32), np.zeros((2, 0), np.float32), 5):
        with pytest.raises(ValueError, match=r' - ERROR, f0_batch: wav must be \[B, Lmax\]'):
            ev.f0_batch(bad)
    for bad in ([4000], [0, 4000], [4000, 4001], [4000.0, 4000.0]):
        with pytest.raises(ValueError, match=r'f0_batch: lens must be 2 integers in \[1, 4000\]'):
            ev.f0_batch(wav, bad)
    for kw in (dict(sr=0), dict(sr=16000.0), dict(hop_length=0), dict(frame_length=-1), dict(hop_length=True)):
        with pytest.raises(ValueError, match=r'must be a positive integer'):
            ev.f0_batch(wav, **kw)
    for kw in (dict(fmin=0.0), dict(fmin=400.0), dict(fmax=50.0), dict(fmax=16001.0), dict(fmin=float('nan'))):
        with pytest.raises(ValueError, match=r'need 0 < fmin < fmax <= sr'):
            ev.f0_batch(wav, **kw)
    for thr in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r'threshold must lie in \(0, 1\]'):
            ev.f0_batch(wav, threshold=thr)
    with pytest.raises(ValueError, match=r'needs lags up to 1067, the kernel holds 1022'):
        ev.f0_batch(wav, fmin=15.0)
    with pytest.raises(ValueError, match=r'frame_length at most 2048'):
        ev.f0_batch(wav, frame_length=4096)
    f0 = np.zeros((2, 51), np.float32)
    with pytest.raises(ValueError, match=r'f0_a must be \[B, F\]'):
        ev.f0_metrics_batch(f0[0], f0, [51, 51], [51, 51])
    with pytest.raises(ValueError, match=r'agree in B'):
        ev.f0_metrics_batch(f0, f0[:1], [51, 51], [51])
    with pytest.raises(ValueError, match=r'len_b must be 2 integers in \[1, 51\]'):
        ev.f0_metrics_batch(f0, f0, [51, 51], [51, 52])
    with pytest.raises(ValueError, match=r'path and path_len together'):
        ev.f0_metrics_batch(f0, f0, [51, 51], [51, 51], path=np.zeros((2, 101, 2), np.int32))
    with pytest.raises(ValueError, match=r'must be int32 tensors'):
        ev.f0_metrics_batch(f0, f0, [51, 51], [51, 51], path=np.zeros((2, 101, 2), np.int32), path_len=np.zeros(2, np.int32))
    import torch
    with pytest.raises(ValueError, match=r'path must be \[B, P, 2\]'):
        ev.f0_metrics_batch(f0, f0, [51, 51], [51, 51], path=torch.zeros((2, 101), dtype=torch.int32), path_len=torch.zeros(2, dtype=torch.int32))
    big = np.zeros((2, 48000), np.float32)
    with pytest.raises(ValueError, match=r'cfg_d .* is required'):
        ev.score_wav_batch(big, None, big, None, None)
    with pytest.raises(ValueError, match=r'wav_b must be \[B, Lmax\]'):
        ev.score_wav_batch(big, None, big[0], None, CFG)
    with pytest.raises(ValueError, match=r'same number of utterances'):
        ev.score_wav_batch(big, None, big[:1], None, CFG)
    with pytest.raises(ValueError, match=r"align must be 'dtw' or 'frame'"):
        ev.score_wav_batch(big, None, big, None, CFG, align='x')
    with pytest.raises(ValueError, match=r'score_wav_batch: need 0 < fmin < fmax <= sr'):
        ev.score_wav_batch(big, None, big, None, CFG, fmin=500.0)
    with pytest.raises(ValueError, match=r'res_type'):
        ev.score_wav_batch(big, None, big, None, CFG, wav_sr_a=48000, res_type='sinc')
    # a valid call reaches the device check
    import _vc
    if not torch.cuda.is_available():
        for call in (lambda: ev.f0_batch(wav, [4000, 1]), lambda: ev.f0_batch(wav, sr=8000, hop_length=40, fmin=30.0, fmax=300.0),
                     lambda: ev.f0_metrics_batch(f0, f0, [51, 3], [1, 51]),
                     lambda: ev.f0_metrics_batch(f0, f0, [51, 3], [1, 51], path=torch.zeros((2, 101, 2), dtype=torch.int32),
                                                 path_len=torch.zeros(2, dtype=torch.int32)),
                     lambda: ev.score_wav_batch(big, [48000, 700], big, None, CFG, wav_sr_a=48000),
                     lambda: ev.score_wav_batch(big, None, big, None, CFG, align='frame')):
            with pytest.raises(_vc.VCError, match='needs a GPU'):
                call()


def test_new_exports_are_declared_exported_and_bound():
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    assert int(re.search(r'#define\s+VC_ABI_VERSION\s+(\d+)', hdr).group(1)) == 7 == _vc.VC_ABI_VERSION
    lib = _vc.lib()
    assert lib.vc_version() == 7
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('vc_f0_yin_f32', 'vc_f0_metrics_f32'):
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
        assert name in _vc._SIGS and hasattr(lib, name)
    assert list(_vc._SIGS)[-2:] == ['vc_f0_yin_f32', 'vc_f0_metrics_f32']           # appended: older names keep their order
    und = __import__('subprocess').run(['nm', '-D', '--undefined-only', _vc.LIB_PATH], capture_output=True, text=True).stdout
    assert 'getenv' not in und


def test_entry_points_refuse_impossible_sizes_before_any_hip_call():
    """No GPU here: a refusal that came after a HIP call would report VC_ERR_HIP (2), not INVALID (1) / UNSUPPORTED (4)."""
    import _vc
    lib = _vc.lib()
    p = ctypes.c_void_p(4096)

    def yin(wav=p, batch=2, max_len=80000, ld=80000, sr=16000.0, hop=80, W=512, tau_min=40, tau_max=267, thr=0.15, f0=p, ap=p,
            max_frames=1001):
        return lib.vc_f0_yin_f32(wav, p, batch, max_len, ld, sr, hop, W, tau_min, tau_max, thr, f0, ap, max_frames, None)

    for kw in (dict(wav=None), dict(f0=None), dict(ap=None)):
        assert yin(**kw) == 1 and b'vc_f0_yin_f32: NULL' in lib.vc_last_error(), kw
    for kw in (dict(batch=0), dict(max_len=0), dict(ld=79999), dict(hop=0), dict(W=0), dict(batch=-1)):
        assert yin(**kw) == 1 and b'vc_f0_yin_f32: bad shape' in lib.vc_last_error(), kw
    for kw in (dict(tau_min=0), dict(tau_min=268), dict(tau_max=-1)):
        assert yin(**kw) == 1 and b'tau_min <= tau_max' in lib.vc_last_error(), kw
    for kw in (dict(sr=0.0), dict(sr=float('inf')), dict(thr=0.0), dict(thr=1.5), dict(thr=float('nan'))):
        assert yin(**kw) == 1 and b'sample_rate > 0 and 0 < threshold' in lib.vc_last_error(), kw
    assert yin(max_frames=1000) == 1 and b'max_frames 1000 is less than' in lib.vc_last_error()
    assert yin(max_frames=0) == 1
    for kw in (dict(batch=65536), dict(W=2049), dict(tau_max=1023), dict(hop=65537), dict(max_len=2 ** 30 + 1, ld=2 ** 30 + 1),
               dict(max_frames=2 ** 30 + 2), dict(max_frames=2 ** 31 - 1)):
        assert yin(**kw) == 4 and b'vc_f0_yin_f32: limits' in lib.vc_last_error(), kw                     # VC_ERR_UNSUPPORTED

    def met(a=p, batch=2, max_a=100, max_b=120, path=p, plen=p, max_path=219, counts=p, values=p):
        return lib.vc_f0_metrics_f32(a, p, p, p, batch, max_a, max_b, path, plen, max_path, counts, values, None)

    for kw in (dict(a=None), dict(counts=None), dict(values=None)):
        assert met(**kw) == 1 and b'vc_f0_metrics_f32: NULL' in lib.vc_last_error(), kw
    for kw in (dict(batch=0), dict(max_a=0), dict(max_b=-5)):
        assert met(**kw) == 1 and b'vc_f0_metrics_f32: bad shape' in lib.vc_last_error(), kw
    for kw in (dict(path=None), dict(plen=None), dict(max_path=0), dict(path=None, plen=None, max_path=5)):
        assert met(**kw) == 1 and b'together' in lib.vc_last_error(), kw
    for kw in (dict(batch=65536), dict(max_a=2 ** 30 + 1), dict(max_path=2 ** 30 + 1)):
        assert met(**kw) == 4 and b'vc_f0_metrics_f32: limits' in lib.vc_last_error(), kw


def test_the_tracker_keeps_its_registers():
    """f0_yin_kernel runs up to 1,024 lanes per workgroup (128 registers per lane at most): the compiler's own report must
    say no spills and no scratch for both kernels of csrc/vc_f0.hip.  The compiler and its flags are the Makefile's own
    (the command `make -n` prints for vc_f0.o), so the report is of the compilation that ships."""
    import shlex
    import subprocess
    csrc = os.path.join(ROOT, 'speech-cloner_amd', 'csrc')
    dry = subprocess.run(['make', '-C', csrc, '-n', '-B', 'vc_f0.o', 'ARCH=gfx950'], capture_output=True, text=True)
    assert dry.returncode == 0, dry.stderr
    line = [ln for ln in dry.stdout.splitlines() if 'vc_f0.hip' in ln and ' -c ' in ln]
    assert len(line) == 1, dry.stdout
    cmd = shlex.split(line[0])
    k = cmd.index('-o')
    cmd = cmd[:k] + cmd[k + 2:] + ['--cuda-device-only', '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage']
    out = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = out.stderr.split('Function Name:')
    for kern in ('f0_yin_kernel', 'f0_metrics_kernel'):
        mine = [b for b in blocks if kern in b.splitlines()[0]]
        assert mine, 'no resource report for %s' % kern
        assert int(re.search(r'VGPRs Spill: (\d+)', mine[0]).group(1)) == 0, mine[0]
        assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', mine[0]).group(1)) == 0, mine[0]
