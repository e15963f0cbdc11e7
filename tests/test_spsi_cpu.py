"""Host side of the deterministic Griffin-Lim phase start (vc_phase_spsi, audio_lib.phase_spsi; no GPU): the reference's
forms against one another, hand-made ownership cases, the exports and their argument checks, the accepted names of
phase0= / phase=, and the gain over a random start on the float64 reference Griffin-Lim."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import fgla_ref as fr
import spsi_ref as sr
from oracle import vocoder_oracle as vo

F_SYN = 200


@pytest.fixture(scope='module')
def voiced():
    """|STFT| of the synthetic voiced signal at 400 / 80, 200 frames: ([bins, F] float64, [F, bins] float32)."""
    a = sr.voiced_magnitudes(F_SYN, 400, 80)
    return a, np.ascontiguousarray(a.T, dtype=np.float32)


@pytest.mark.parametrize('chunk', [1, 7, 32, F_SYN + 1])
def test_chunked_form_equals_the_sequential_one_bit_for_bit(voiced, chunk):
    amp = voiced[1]
    assert np.array_equal(sr.phase_chunked(amp, 400, 80, chunk), sr.phase_sequential(amp, 400, 80))
    # and with a short utterance inside a longer slab: zeros beyond, the same bits before
    got = sr.phase_chunked(amp, 400, 80, chunk, n_frames=45)
    assert np.array_equal(got[:45], sr.phase_sequential(amp[:45], 400, 80)) and not got[45:].any()


def test_fixed_point_stays_with_the_float64_form(voiced):
    """200 frames: the fixed-point increment is off by at most 2^-32 turn (floor of the whole part) + 2^-33 turn (rint of
    the fractional part) per frame, 200 * 1.5 * 2^-32 * 2 pi = 4.4e-7 rad, plus half a float32 ulp of pi (1.2e-7) in the
    output: well inside the 1e-5 rad asked for."""
    amp = voiced[1]
    d = sr.wrapped_distance(sr.phase_sequential(amp, 400, 80), sr.phase_float64(amp, 400, 80))
    print('wrapped distance fixed point vs float64: %.3e rad' % d)
    assert d <= 1e-5


OWNERSHIP = [
    # magnitudes                          owners (-1: unowned)
    ([0, 1, 3, 1, 0],                     [-1, 2, 2, 2, -1]),               # one peak owns both slopes; ends unowned
    ([0, 2, 1, 3, 0],                     [-1, 1, 3, 3, -1]),               # valley bin 2: the higher-frequency peak
    ([5, 4, 3, 4, 5, 4, 6],               [-1, -1, 4, 4, 4, 4, -1]),        # bin 1 falls from bin 0, bin 5 rises to bin 6: edges are no peaks
    ([1, 1, 1, 1, 1],                     [-1, -1, -1, -1, -1]),            # all equal
    ([0, 1, 2, 3, 4],                     [-1, -1, -1, -1, -1]),            # rising ramp: reaches nb-1, not a peak
    ([4, 3, 2, 1, 0],                     [-1, -1, -1, -1, -1]),            # falling ramp
    ([0, 3, 1, 1, 0],                     [-1, 1, 1, -1, -1]),              # plateau 1,1: bin 3 is not below bin 2
    ([0, 1, 2, 2, 1, 0],                  [-1, -1, -1, -1, -1, -1]),        # flat top: no strict peak at all
    ([9, 1, 0, 0, 0, 2, 9],               [-1, -1, -1, -1, -1, -1, -1]),    # maxima on the edge bins are not peaks
    ([0, 5, 0, 0, 0, 0, 0],               [-1, 1, 1, -1, -1, -1, -1]),      # single peak at bin 1
    ([0, 0, 0, 0, 0, 5, 0],               [-1, -1, -1, -1, 5, 5, -1]),      # single peak at nb-2
    ([0, 1, 2, 5, 4, 3, 3, 7, 1],         [-1, 3, 3, 3, 3, 3, 7, 7, -1]),   # tie 3, 3: bin 5 falls from 3, bin 6 rises to 7
]


@pytest.mark.parametrize('case', range(len(OWNERSHIP)))
def test_hand_made_ownership(case):
    m, want = OWNERSHIP[case]
    m = np.asarray(m, dtype=np.float32)
    assert list(sr.owners(m)) == want
    assert list(sr.owners_literal(m)) == want


def test_ownership_forms_agree_on_ties_and_nan():
    rng = np.random.RandomState(0)
    for trial in range(200):
        nb = int(rng.randint(3, 24))
        m = rng.randint(0, 4, nb).astype(np.float32) if trial % 2 else rng.rand(nb).astype(np.float32)
        if trial % 5 == 0:
            m[rng.randint(nb)] = np.nan
        assert np.array_equal(sr.owners(m), sr.owners_literal(m)), m
    assert (sr.owners(np.full(9, np.nan, np.float32)) == -1).all()


def test_increment_arithmetic():
    """A symmetric peak has p = 0: the increment is the whole part alone; a half turn per frame at hop * k = n_fft / 2."""
    m = np.array([0, 1, 4, 1, 0, 0, 0, 0, 0], dtype=np.float32)              # nb 9: n_fft 16
    inc = sr.increments(m, 16, 4)
    assert inc[2] == (((4 * 2) % 16) << 32) // 16 == 1 << 31
    src, off = sr.frame_map(m, 16, 4)
    assert list(src) == [0, 2, 2, 2, 2, 5, 6, 7, 8]                          # bin 4 falls from the peak over bin 3
    assert list(off) == [0, 0, 1 << 31, 0, 1 << 31, 0, 0, 0, 0]              # odd neighbours: half turn + half turn wraps to 0
    # an asymmetric peak: p = 0.5 * (1 - 2) / (1 - 8 + 2) = 0.1 (float32), frac = rint(float64(p) * 2^30)
    m[3] = 2
    p = np.float32(0.5) * np.float32(-1) / np.float32(-5)
    assert sr.peak_offset(m, 16, 4)[2] == p
    assert sr.increments(m, 16, 4)[2] == ((1 << 31) + int(np.rint(np.float64(p) * 2.0 ** 30))) % (1 << 32)
    # outside the expected inputs: a non-finite or large p counts as 0
    bad = np.array([-np.inf, np.inf, 0, 1, 0], dtype=np.float32)
    assert sr.peak_offset(bad, 8, 2)[1] == 0


def test_exports_and_abi():
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    assert re.search(r'#define VC_ABI_VERSION 7\b', hdr) and _vc.VC_ABI_VERSION == 7
    assert 'vc_phase_spsi_workspace_bytes(int32_t batch, int32_t max_frames, int32_t n_bins);' in hdr
    assert re.search(r'int vc_phase_spsi\(const float\* d_amp, const int32_t\* d_n_frames, int32_t batch', hdr)
    assert 'finite and non-negative' in hdr
    assert _vc._SIGS['vc_phase_spsi_workspace_bytes'] == (C.c_size_t, [C.c_int32] * 3)
    res, args = _vc._SIGS['vc_phase_spsi']
    assert res is C.c_int and len(args) == 11 and args[2:7] == [C.c_int32] * 5 and args[9] is C.c_size_t
    lib = _vc.lib()
    assert lib.vc_version() == 7
    assert lib.vc_phase_spsi.argtypes == args and lib.vc_phase_spsi_workspace_bytes.restype is C.c_size_t


def test_workspace_steps_with_the_chunk_length():
    """10 bytes per bin and chunk (offset, state, source), each section rounded to 256: the chunk length the Python side
    names is the one the library counts with."""
    import _vc
    import audio_lib
    lib = _vc.lib()
    Ck = audio_lib.SPSI_CHUNK_FRAMES
    assert Ck == 32
    w = lambda F, B=1, nb=256: lib.vc_phase_spsi_workspace_bytes(B, F, nb)
    assert w(1) == w(Ck) == 256 * 10 and w(Ck + 1) == w(2 * Ck) == 2 * 256 * 10 and w(2 * Ck + 1) == 3 * 256 * 10
    assert w(Ck, B=3) == 3 * 256 * 10
    e = 16 * 32 * 201
    assert lib.vc_phase_spsi_workspace_bytes(16, 1000, 201) == 2 * (-(-e * 4 // 256) * 256) + (-(-e * 2 // 256) * 256)
    assert w(0) == 0 and w(5, B=0) == 0 and w(5, nb=0) == 0


def test_bad_arguments_are_errors_before_any_launch():
    """No device here: every one of these returns VC_ERR_INVALID (1) before the first launch, so nothing dereferences the
    pointers."""
    import _vc
    lib = _vc.lib()
    p = C.c_void_p(256)                                                      # never dereferenced
    need = lib.vc_phase_spsi_workspace_bytes(2, 40, 201)
    good = dict(amp=p, nf=None, B=2, F=40, nb=201, n_fft=400, hop=80, out=p, ws=p, wsb=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.vc_phase_spsi(a['amp'], a['nf'], a['B'], a['F'], a['nb'], a['n_fft'], a['hop'], a['out'], a['ws'], a['wsb'], None)
        return rc, lib.vc_last_error()

    for kw in (dict(amp=None), dict(out=None), dict(ws=None), dict(B=0), dict(B=65536), dict(F=0), dict(nb=200), dict(nb=202),
               dict(n_fft=2, nb=2), dict(n_fft=131072, nb=65537), dict(n_fft=131068, nb=65535), dict(n_fft=8000, nb=4001),
               dict(hop=0), dict(hop=65536), dict(wsb=need - 1), dict(wsb=0)):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(b'vc_phase_spsi:'), (kw, rc, msg)
    assert b'65535' in call(n_fft=131072, nb=65537)[1]
    assert b'workspace' in call(wsb=need - 1)[1]
    assert b'NULL' in call(amp=None)[1]


def test_unknown_phase_names_list_spsi():
    import audio_lib
    import conversion
    amp = np.ones((1, 20, 201), np.float32)
    with pytest.raises(ValueError, match="'spsi'"):
        audio_lib.griffin_lim_batch(amp, None, 400, 80, 3, phase0='nope')
    with pytest.raises(ValueError, match="'spsi'"):
        audio_lib.from_power_to_wav_batch(amp, None, hop_length=80, win_length=400, n_iter=3, phase0='nope')
    with pytest.raises(ValueError, match="'spsi'"):
        conversion.convert_batch(None, np.zeros((1, 16000), np.float32), None, dict(n_fft=None, win_length=400), phase='nope')
    with pytest.raises(ValueError, match='phase_spsi: amp must be'):
        audio_lib.phase_spsi(np.ones((1, 20, 200), np.float32), None, 80, 400)
    with pytest.raises(ValueError, match='phase_spsi: n_frames'):
        audio_lib.phase_spsi(amp, [21], 80, 400)
    with pytest.raises(ValueError, match='phase_spsi: n_frames'):
        audio_lib.phase_spsi(amp, [3, 4], 80, 400)


@pytest.mark.parametrize('proj', [4, 8, 16])
def test_spsi_start_beats_a_random_start_on_the_reference_loop(voiced, proj):
    """The sanity condition on the input of the GPU convergence test, not a claim about the device: on the float64
    reference Griffin-Lim at momentum 0.99 the SPSI start's spectral convergence is at most 0.7 x the random start's."""
    a64, a32 = voiced
    spsi = sr.phase_sequential(a32, 400, 80).T.astype(np.float64)
    rand = vo.initial_phase(a64.shape, 0)
    sc = [fr.sc(fr.griffin_lim_momentum(a64, 400, 80, proj + 1, 0.99, phase0=ph), a64, 400, 80) for ph in (spsi, rand)]
    print('projections %d: SC spsi %.4f random %.4f ratio %.3f' % (proj, sc[0], sc[1], sc[0] / sc[1]))
    assert sc[0] <= 0.7 * sc[1]
