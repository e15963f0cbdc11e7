"""Fast Griffin-Lim without a GPU: the CPU reference (tests/fgla_ref.py) against the oracle's plain
loop and on convergence, the momentum argument's validation, and how conversion / conversion2 hand
it to a vocoder callable."""
import math

import numpy as np
import pytest

import fgla_ref as fr
from oracle import frontend_oracle as fo
from oracle import vocoder_oracle as vo


def _amp_of_speech(L, seed, n_fft=400, hop=80, win=400):
    y = fo.synth_speech(1, L, seed=seed)[0].astype(np.float64)
    y = y[:hop * (len(y) // hop)]
    return np.abs(vo.stft(y, n_fft, hop, win)).astype(np.float64)          # [bins, F]


def test_reference_at_zero_momentum_is_the_oracle_bit_for_bit():
    amp = _amp_of_speech(8000, 11)
    ph = vo.initial_phase(amp.shape, 3)
    for n in (1, 2, 5):
        tr_a, tr_b = [], []
        a = vo.griffin_lim_alg(amp, 400, 80, num_iters=n, phase0=ph, trace=tr_a)
        b = fr.griffin_lim_momentum(amp, 400, 80, n, 0.0, phase0=ph, trace=tr_b)
        assert a.dtype == b.dtype == np.float64 and np.array_equal(a, b)
        assert tr_a == tr_b


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_two_or_fewer_iterations_do_not_depend_on_momentum(dtype):
    amp = _amp_of_speech(8000, 5)
    ph = vo.initial_phase(amp.shape, 1)
    for n in (1, 2):
        base = fr.griffin_lim_momentum(amp, 400, 80, n, 0.0, phase0=ph, dtype=dtype)
        for m in (0.5, 0.99):
            assert np.array_equal(fr.griffin_lim_momentum(amp, 400, 80, n, m, phase0=ph, dtype=dtype), base)
    # from the third iteration on the momentum acts
    assert not np.array_equal(fr.griffin_lim_momentum(amp, 400, 80, 3, 0.99, phase0=ph),
                              fr.griffin_lim_momentum(amp, 400, 80, 3, 0.0, phase0=ph))


def test_float32_mode_stays_near_float64():
    amp = _amp_of_speech(8000, 11)
    ph = vo.initial_phase(amp.shape, 3)
    a = fr.griffin_lim_momentum(amp, 400, 80, 8, 0.99, phase0=ph)
    b = fr.griffin_lim_momentum(amp, 400, 80, 8, 0.99, phase0=ph, dtype=np.float32)
    assert b.dtype == np.float32 and 0.0 < fr.rel_l2(b, a) < 1e-4


@pytest.mark.parametrize('seed', [3, 7])
def test_momentum_reaches_plain_convergence_in_fewer_iterations(seed):
    """Spectral convergence of synthetic speech (301 frames, n_fft 400, hop 80, phase seed 0).
    Measured: seed 3  SC(0, 200) 0.0667, SC(0.99, 32) 0.0653 (0.98x), SC(0.99, 50) 0.0372 (0.56x);
              seed 7  SC(0, 200) 0.1080, SC(0.99, 32) 0.1038 (0.96x), SC(0.99, 50) 0.0712 (0.66x)."""
    amp = _amp_of_speech(24000, seed)
    assert amp.shape == (201, 301)
    ph = vo.initial_phase(amp.shape, 0)

    def sc(m, n):
        return fr.sc(fr.griffin_lim_momentum(amp, 400, 80, n, m, phase0=ph), amp, 400, 80)

    plain = sc(0.0, 200)
    assert sc(0.99, 50) <= 0.85 * plain
    assert sc(0.99, 32) <= 1.1 * plain


BAD = [-0.1, 1.0, 1.5, float('nan'), float('inf'), -float('inf')]


@pytest.mark.parametrize('bad', BAD)
def test_bad_momentum_raises_before_the_gpu(bad):
    """Validated first: no GPU, native library call or draw from the global generator happens."""
    import audio_lib
    amp = np.ones((3, 50, 201), np.float32)
    with pytest.raises(ValueError, match='momentum'):
        audio_lib.griffin_lim_batch(amp, None, 400, 80, 4, momentum=bad)
    with pytest.raises(ValueError, match='momentum'):
        audio_lib.from_power_to_wav_batch(amp, None, hop_length=80, win_length=400, n_iter=4, momentum=bad)
    np.random.seed(4)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match='momentum'):
        audio_lib.griffin_lim_alg(amp[0].T, 400, 80, num_iters=4, verbose=False, momentum=bad)
    with pytest.raises(ValueError, match='momentum'):
        audio_lib.from_power_to_wav(amp[0], hop_length=80, win_length=400, n_iter=4, verbose=False, momentum=bad)
    assert np.array_equal(np.random.get_state()[1], state)


def test_momentum_range_is_torchaudios():
    import audio_lib
    assert audio_lib.check_momentum(0) == 0.0
    assert audio_lib.check_momentum(0.99) == 0.99
    assert audio_lib.check_momentum(np.float32(0.5)) == 0.5
    assert audio_lib.check_momentum(math.nextafter(1.0, 0.0)) < 1.0


# ------------------------------------------------------------------ conversion drivers
_CFG = {'hop_length': 80, 'n_timesteps': 400, 'sample_rate': 16000, 'win_length': 400, 'n_fft': None,
        'P_dB_norm_factor': 0.01, 'pre_emphasis': 0.97, 'mean_abs_amp_norm': 0.003}
_OLD_KEYS = {'realse', 'P_dB_norm_factor', 'pre_emphasis', 'hop_length', 'win_length', 'mean_abs_amp_norm', 'n_iter',
             'n_fft'}


class _StubDecoder:
    def __init__(self):
        self.calls = 0

    def predict(self, x, batch_size=32):
        from collections import namedtuple
        self.calls += 1
        nt = namedtuple('predict', 'y_mel y_stft y_phn')
        return nt(x[..., :3] * 2.0, x[..., :5] + 1.0, x[..., :4] - 1.0)


class _RefSignatureVocoder:
    """audio_lib.from_power_to_wav's signature as the reference has it: no ``momentum`` parameter."""

    def __init__(self):
        self.calls = []

    def __call__(self, P, P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=40, win_length=800,
                 mean_abs_amp_norm=0.01, n_iter=200, n_fft=None, realse=1.0):
        self.calls.append(dict(P_dB_norm_factor=P_dB_norm_factor, pre_emphasis=pre_emphasis, hop_length=hop_length,
                               win_length=win_length, mean_abs_amp_norm=mean_abs_amp_norm, n_iter=n_iter,
                               n_fft=n_fft, realse=realse))
        return np.zeros(3)


class _KwVocoder:
    def __init__(self):
        self.kwargs = []

    def __call__(self, P, **kw):
        self.kwargs.append(kw)
        return np.ones(2)


def _inputs(F=801):
    rng = np.random.RandomState(2)
    return rng.standard_normal((F, 80)), rng.standard_normal((F, 80)), rng.standard_normal((F, 201))


@pytest.mark.parametrize('driver', ['conversion', 'conversion2'])
def test_zero_momentum_calls_a_reference_signature_vocoder_with_the_old_keywords(driver):
    import conversion
    voc, kwv = _RefSignatureVocoder(), _KwVocoder()
    r = getattr(conversion, driver)(_StubDecoder(), *_inputs(), _CFG, t_s=0, t_e=60, n_iter=7, vocoder=voc)
    assert len(voc.calls) == 2 and r.y_wav_pred is not None
    getattr(conversion, driver)(_StubDecoder(), *_inputs(), _CFG, t_s=0, t_e=60, n_iter=7, vocoder=kwv, momentum=0.0)
    assert [set(k) for k in kwv.kwargs] == [_OLD_KEYS, _OLD_KEYS]


@pytest.mark.parametrize('driver', ['conversion', 'conversion2'])
def test_momentum_is_passed_to_the_vocoder(driver):
    import conversion
    kwv = _KwVocoder()
    getattr(conversion, driver)(_StubDecoder(), *_inputs(), _CFG, t_s=0, t_e=60, n_iter=32, vocoder=kwv,
                                momentum=0.99, giffin_lim_input=True)
    assert len(kwv.kwargs) == 2
    for kw in kwv.kwargs:
        assert set(kw) == _OLD_KEYS | {'momentum'} and kw['momentum'] == 0.99 and kw['n_iter'] == 32
    with pytest.raises(TypeError):                     # a reference-signature callable cannot take it
        getattr(conversion, driver)(_StubDecoder(), *_inputs(), _CFG, t_s=0, t_e=60, vocoder=_RefSignatureVocoder(),
                                    momentum=0.5)


@pytest.mark.parametrize('driver', ['conversion', 'conversion2'])
def test_conversion_rejects_bad_momentum_before_the_decoder(driver):
    import conversion
    dec, kwv = _StubDecoder(), _KwVocoder()
    for bad in BAD:
        with pytest.raises(ValueError, match='momentum'):
            getattr(conversion, driver)(dec, *_inputs(), _CFG, t_s=0, t_e=60, vocoder=kwv, momentum=bad)
    assert dec.calls == 0 and not kwv.kwargs
