"""Host side of conversion.convert_batch (no GPU): the Philox reference against published vectors, the tables of
``convert_plan`` against the oracle's framing, the closed form the stitch kernel implements against
``conversion.compound_index``, entry validation, and the ABI of the three new exports."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import conversion_oracle as co
import philox_ref

CFG = dict(sample_rate=16000, hop_length=80, n_timesteps=400, win_length=400, n_fft=None, pre_emphasis=0.97,
           n_mels=80, n_mfcc=40, window='hann', mfcc_normaleze_first_mfcc=True, mfcc_norm_factor=0.01,
           calc_mfcc_derivate=True, M_dB_norm_factor=0.01, P_dB_norm_factor=0.01, mean_abs_amp_norm=0.003,
           clip_output=True)


def test_philox4x32_10_known_answers():
    """Random123's published known-answer vectors (kat_vectors: philox4x32 10)."""
    kat = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for ctr, key, want in kat:
        got = ' '.join('%08x' % int(w) for w in philox_ref.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, got)


def test_phase_ref_addressing():
    a = philox_ref.phase_ref(7, 5, 9, 201)
    assert a.dtype == np.float32 and a.shape == (9, 201) and a.min() >= 0.0 and a.max() < np.float32(np.pi)
    # a longer utterance with the same id starts with the same values; another id or seed does not
    assert np.array_equal(philox_ref.phase_ref(7, 5, 30, 201)[:9], a)
    assert not np.array_equal(philox_ref.phase_ref(7, 6, 9, 201), a)
    assert not np.array_equal(philox_ref.phase_ref(8, 5, 9, 201), a)
    assert not np.array_equal(philox_ref.phase_ref(7 + (1 << 32), 5, 9, 201), a)
    # element e is word e % 4 of block e // 4
    w = philox_ref.philox4x32_10((3, 5, 0, 0), (7, 0))
    e = 3 * 4 + 2
    assert a.reshape(-1)[e] == np.float32(np.pi) * (np.float32(int(w[2]) >> 8) * np.float32(2.0 ** -24))


# ---- numpy emulation of the two kernels, driven by the tables only (include/vc_hip.h)
def emu_cut(src, win_tab, n_frames, T):
    B, Fmax, C = src.shape
    out = np.full((len(win_tab), T, C), np.nan, dtype=src.dtype)
    for w, (u, f0) in enumerate(win_tab):
        for t in range(T):
            f = f0 + t
            out[w, t] = src[u, f] if f < min(n_frames[u], Fmax) else 0
    return out


def stitch_source(t, T, N, w0, w1):
    """(window, frame) in the window batch of output row t, None for a zero row: the header's closed form."""
    q, h = T // 4, T // 2
    if t >= N * T:
        return None
    if N == 1 or w1 < 0:
        return w0 + t // T, t % T
    if t < T - q:
        return w0, t
    if t >= N * T - (T - q):
        return w0 + N - 1, t - (N - 1) * T
    j, r = divmod(t - (T - q), h)
    return (w1 + j // 2, q + r) if j % 2 == 0 else (w0 + (j + 1) // 2, q + r)


def emu_stitch(src, utt_tab, Fout):
    W, T, C = src.shape
    out = np.full((len(utt_tab), Fout, C), np.nan, dtype=np.float32)
    for b, (w0, w1, N) in enumerate(utt_tab):
        for t in range(Fout):
            s = stitch_source(t, T, N, w0, w1)
            out[b, t] = 0 if s is None else src[s]
    return out


@pytest.mark.parametrize('T', [400, 8])
def test_closed_form_is_compound_index(T):
    import conversion
    for N in range(2, 7):
        which, win, frame = conversion.compound_index(N, T)
        assert len(which) == N * T
        w0, w1 = 3, 11
        for t in range(N * T):
            want = ((w1 if which[t] else w0) + win[t], frame[t])
            assert stitch_source(t, T, N, w0, w1) == want, (N, T, t)
        assert stitch_source(N * T, T, N, w0, w1) is None
    # one window (or one pass) is the reshape; compound_index(1, T) is NOT (it returns 1.5 T rows)
    assert len(conversion.compound_index(1, T)[0]) == T + T // 2
    assert [stitch_source(t, T, 1, 4, -1) for t in range(T)] == [(4, t) for t in range(T)]
    assert [stitch_source(t, T, 3, 4, -1) for t in range(3 * T)] == [(4 + t // T, t % T) for t in range(3 * T)]


CASES = [  # (frame counts, t_s, t_e)
    ([300, 799, 1001, 2000], 0, 60),          # N = 1, 2, 3, 5
    ([400, 800, 1200], 0, 60),                # exact multiples of 400: no padding
    ([1001, 1700, 2400], 1, 60),              # t_s > 0: n_s = 200
    ([1001, 2300, 500], 0, 10),               # t_e = 10 s = 2000 frames cuts the 2300-frame utterance short
    ([1001, 1300], 2, 12),
]


@pytest.mark.parametrize('frames,t_s,t_e', CASES)
@pytest.mark.parametrize('two_pass', [True, False])
def test_tables_reproduce_the_oracle_framing(frames, t_s, t_e, two_pass):
    """cut + (stand-in model: identity on a few columns) + stitch driven by convert_plan's tables equals, per utterance,
    the oracle's window_plan + zero padding + compound, exactly."""
    import conversion
    T, C = 400, 3
    lens = [80 * (f - 1) + 17 for f in frames]                     # 1 + len // 80 == f
    plan = conversion.convert_plan(lens, CFG, t_s, t_e, two_pass)
    assert list(plan.n_src) == frames and plan.B == len(frames)
    rng = np.random.RandomState(1)
    Fmax = max(frames) + 3
    src = rng.standard_normal((len(frames), Fmax, C)).astype(np.float32)
    for b, f in enumerate(frames):
        src[b, f:] = 0.0                                           # the front-end's rows beyond an utterance are zero
    x = emu_cut(src, plan.win_tab, plan.n_clip, T)
    assert not np.isnan(x).any() and x.shape == (plan.W, T, C)
    got = emu_stitch(x, plan.utt_tab, plan.Fout)
    true = emu_cut(src, plan.true_tab, plan.n_clip, plan.Fout)
    assert not np.isnan(got).any() and not np.isnan(true).any()
    for b, f in enumerate(frames):
        total, n_s, n_e = co.window_plan(f, 16000, 80, T, t_s, t_e)
        assert (plan.n_s[b], plan.n_e[b]) == (n_s, n_e) and plan.n_out[b] == n_e - n_s == plan.N[b] * T
        padded = np.concatenate([src[b, :f], np.zeros((total - f, C), np.float32)], 0)
        y0 = padded[n_s:n_e].reshape(-1, T, C)
        if two_pass and n_e - n_s > T:
            y1 = padded[n_s + T // 2:n_e - T // 2].reshape(-1, T, C)
            want = co.compound(y0, y1)
        else:
            want = y0.reshape(-1, C)
        n = n_e - n_s
        assert np.array_equal(got[b, :n], want) and not got[b, n:].any()
        assert np.array_equal(true[b, :n], padded[n_s:n_e]) and not true[b, n:].any()
    assert plan.Fout == max(plan.n_out)


class _NoDecoder:
    encoder = object()

    def __getattr__(self, name):
        raise AssertionError('the decoder was touched before validation finished')


def test_validation_happens_before_any_gpu_work():
    """No GPU here: a call that got past its checks would fail with VCError('... needs a GPU'), not with these."""
    import conversion
    import audio_lib
    wav = np.zeros((3, 80000), np.float32)
    ok = dict(cfg_d=CFG, lens=[80000, 40000, 60000])
    with pytest.raises(Exception, match=r'n_e <= n_s.*utterance 1'):
        conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[80000, 30000, 60000], t_s=2)   # 376 -> 400 frames, n_s = 400
    with pytest.raises(Exception, match=r'n_e <= n_s.*utterance 2'):
        conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[80000, 80000, 30000], t_s=2)
    for bad in (1.0, -0.1, float('nan'), 1.5):
        with pytest.raises(ValueError, match='momentum'):
            conversion.convert_batch(_NoDecoder(), wav, momentum=bad, **ok)
    with pytest.raises(ValueError, match='phase'):
        conversion.convert_batch(_NoDecoder(), wav, phase='host', **ok)
    with pytest.raises(ValueError, match='phase'):
        conversion.convert_batch(_NoDecoder(), wav, phase=np.zeros((3, 400, 201), np.float32), **ok)   # Fout is 1200
    with pytest.raises(ValueError, match='utt_ids'):
        conversion.convert_batch(_NoDecoder(), wav, utt_ids=[0, 1], **ok)
    with pytest.raises(ValueError, match='lens'):
        conversion.convert_batch(_NoDecoder(), wav, cfg_d=CFG, lens=[80000, 90000, 100])
    with pytest.raises(ValueError, match='seed'):
        conversion.convert_batch(_NoDecoder(), wav, seed=-1, **ok)
    with pytest.raises(ValueError, match='utt_ids'):
        audio_lib.phase_init([10, 20], 20, 201, 0, utt_ids=[1])
    with pytest.raises(ValueError, match='n_frames'):
        audio_lib.phase_init([10, 30], 20, 201, 0)
    # and a valid call reaches the device check
    import _vc
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_vc.VCError, match='needs a GPU'):
            conversion.convert_batch(_NoDecoder(), wav, **ok)


def test_short_utterance_is_one_padded_window():
    """251 frames, t_s = 0: the reference pads to 400 and converts one window (no error)."""
    import conversion
    plan = conversion.convert_plan([20000], CFG, 0, 60, True)
    assert list(plan.N) == [1] and plan.utt_tab.tolist() == [[0, -1, 1]] and plan.win_tab.tolist() == [[0, 0]]
    assert list(plan.n_clip) == [251] and plan.Fout == 400


def test_new_exports_are_declared_exported_and_bound():
    import _vc
    hdr = open(os.path.join(ROOT, 'include', 'vc_hip.h')).read()
    assert int(re.search(r'#define\s+VC_ABI_VERSION\s+(\d+)', hdr).group(1)) == 7 == _vc.VC_ABI_VERSION
    lib = _vc.lib()
    assert lib.vc_version() == 7
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('vc_cut_windows', 'vc_compound_stitch', 'vc_phase_init'):
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
        assert name in _vc._SIGS and hasattr(lib, name)
    # validation precedes any launch (no GPU needed): NULL pointers, bad shapes, T not a multiple of 4, bad dtype
    p = ctypes.c_void_p(4096)
    assert lib.vc_cut_windows(None, None, None, 1, 1, 1, 400, 80, None, None) == 1 and b'vc_cut_windows' in lib.vc_last_error()
    assert lib.vc_cut_windows(p, p, None, 1, 10, 0, 400, 80, p, None) == 1
    assert lib.vc_compound_stitch(None, 0, None, 1, 1, 400, 80, 400, None, None, 0.0, None) == 1
    assert lib.vc_compound_stitch(p, 0, p, 1, 1, 402, 80, 402, p, None, 0.0, None) == 1 and b'multiple of 4' in lib.vc_last_error()
    assert lib.vc_compound_stitch(p, 2, p, 1, 1, 400, 80, 400, p, None, 0.0, None) == 1 and b'src_dtype' in lib.vc_last_error()
    assert lib.vc_compound_stitch(p, 1, p, 1, 1, 400, 201, 400, p, p, 0.01, None) == 1 and b'float32' in lib.vc_last_error()
    assert lib.vc_compound_stitch(p, 0, p, 1, 1, 400, 201, 400, p, p, 0.0, None) == 1 and b'P_dB_norm_factor' in lib.vc_last_error()
    assert lib.vc_phase_init(None, None, 1, 10, 201, 0, None, None) == 1 and b'vc_phase_init' in lib.vc_last_error()
    assert lib.vc_phase_init(None, None, 0, 10, 201, 0, p, None) == 1
