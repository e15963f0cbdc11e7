"""conversion.convert_batch on the device: the three kernels of csrc/vc_convert.hip bit for bit against numpy, the
whole ragged batch against the oracle chain of test_conversion_gpu.py (same weights, same tolerances), the
device-drawn phase against tests/philox_ref.py, momentum, the bf16 / MX-FP8 decoders, graph replay, and the absence
of host synchronisation inside the call."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import fgla_ref as fr
import philox_ref
from conftest import ROOT
from oracle import conversion_oracle as co
from oracle import frontend_oracle as fo
from oracle import model_oracle as mo
from oracle import vocoder_oracle as vo
from test_conversion_gpu import _cfgs, _fe_kwargs, _oracle_predict
from test_convert_batch_cpu import emu_cut, emu_stitch

pytestmark = pytest.mark.gpu

N_ITER = 4
SECONDS = (3.2, 1.5, 5.0)            # N = 2; N = 1 (reshape fallback); F = 1001 -> padded to 1200, N = 3


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _nan(shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


# --------------------------------------------------------------------------------------------- kernels
def _plan(frames, t_s=0, t_e=60, two_pass=True):
    import conversion
    from test_convert_batch_cpu import CFG
    return conversion.convert_plan([80 * (f - 1) + 5 for f in frames], CFG, t_s, t_e, two_pass)


@pytest.mark.parametrize('C', [80, 61, 201])
def test_cut_windows_bit_exact(C):
    import conversion
    frames = [700, 799, 1001, 2300, 800]
    plan = _plan(frames, t_s=1, t_e=10)                           # n_s = 200; t_e cuts the 2300-frame utterance at 1800
    rng = np.random.RandomState(C)
    src = rng.standard_normal((len(frames), max(frames) + 2, C)).astype(np.float32)      # rows beyond n_clip are NOT zero:
    want = emu_cut(src, plan.win_tab, plan.n_clip, 400)                                  # the kernel must not copy them
    out = _nan((plan.W, 400, C))
    conversion.cut_windows(_dev(src), _dev(plan.win_tab), _dev(plan.n_clip), 400, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    # the one-row-block-per-utterance cut of the true spectra, and a slab that is not a multiple of 4 floats
    for T in (plan.Fout, 7):
        want = emu_cut(src, plan.true_tab, plan.n_clip, T)
        out = _nan((plan.B, T, C))
        conversion.cut_windows(_dev(src), _dev(plan.true_tab), _dev(plan.n_clip), T, out=out)
        assert np.array_equal(out.cpu().numpy(), want), T


@pytest.mark.parametrize('C,dtype', [(80, torch.float32), (61, torch.float32), (61, torch.bfloat16), (64, torch.bfloat16),
                                     (201, torch.float32)])
@pytest.mark.parametrize('two_pass', [True, False])
def test_compound_stitch_bit_exact(C, dtype, two_pass):
    import conversion
    frames = [300, 799, 1001, 2000, 800]
    plan = _plan(frames, two_pass=two_pass)
    assert sorted(set(plan.N)) == [1, 2, 3, 5]
    src = _dev(np.random.RandomState(C).standard_normal((plan.W, 400, C)).astype(np.float32), dtype)
    want = emu_stitch(src.float().cpu().numpy(), plan.utt_tab, plan.Fout)
    out = _nan((plan.B, plan.Fout, C))
    conversion.compound_stitch(src, _dev(plan.utt_tab), plan.Fout, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(got, want)
    if two_pass and dtype == torch.float32:                       # and the oracle's compound itself
        y = src.cpu().numpy()
        for b, (w0, w1, N) in enumerate(plan.utt_tab):
            ref = co.compound(y[w0:w0 + N], y[w1:w1 + N - 1]) if N > 1 else y[w0]
            assert np.array_equal(got[b, :N * 400], ref)


def test_stitch_table_outside_the_batch_gives_zeros():
    import conversion
    src = _dev(np.ones((4, 400, 80), np.float32))
    tab = np.array([[0, 2, 2], [3, -1, 2], [-1, -1, 1], [0, 3, 3]], np.int32)      # rows 1.. point outside 4 windows
    out = _nan((4, 1200, 80))
    conversion.compound_stitch(src, _dev(tab), 1200, out=out)
    got = out.cpu().numpy()
    assert (got[0, :800] == 1).all() and not got[0, 800:].any() and not got[1:].any()


@pytest.mark.parametrize('realse', [1.0, 1.2])
def test_fused_magnitude_equals_compound_then_power_to_amp(realse):
    """realse == 1: the fused flavour.  realse != 1: convert_batch's route, the stitched spectrum through the existing
    vc_power_to_amp launch (bit-identical by construction; include/vc_hip.h says so)."""
    import _vc
    import conversion
    frames = [300, 799, 1001, 2000]
    plan = _plan(frames)
    y = np.random.RandomState(5).uniform(-0.1, 0.9, (plan.W, 400, 201)).astype(np.float32)
    want_P = np.zeros((plan.B, plan.Fout, 201), np.float32)
    for b, (w0, w1, N) in enumerate(plan.utt_tab):
        want_P[b, :N * 400] = co.compound(y[w0:w0 + N], y[w1:w1 + N - 1]) if N > 1 else y[w0]
    want_amp = _nan(want_P.shape)
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(_dev(want_P)), _vc.ptr(_dev(plan.n_out)), plan.B, plan.Fout, 201, 0.01,
                                        realse, _vc.ptr(want_amp), _vc.current_stream()))
    P, amp = _nan(want_P.shape), _nan(want_P.shape)
    if realse == 1.0:
        conversion.compound_stitch(_dev(y), _dev(plan.utt_tab), plan.Fout, P_dB_norm_factor=0.01, out=P, amp=amp)
    else:
        conversion.compound_stitch(_dev(y), _dev(plan.utt_tab), plan.Fout, out=P)
        _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(P), _vc.ptr(_dev(plan.n_out)), plan.B, plan.Fout, 201, 0.01, realse,
                                            _vc.ptr(amp), _vc.current_stream()))
    assert np.array_equal(P.cpu().numpy(), want_P)
    assert torch.equal(amp, want_amp) and float(amp.max()) > 1e-3


def test_phase_init_bit_exact_and_batch_independent():
    import audio_lib
    nf = [400, 1200, 37, 800, 1, 999, 0, 1001]
    ph = audio_lib.phase_init(nf, 1201, 201, seed=11, out=_nan((8, 1201, 201))).cpu().numpy()       # odd slab: scalar stores
    ph4 = audio_lib.phase_init(nf, 1204, 201, seed=11, out=_nan((8, 1204, 201))).cpu().numpy()      # 16-byte stores
    for b, n in enumerate(nf):
        ref = philox_ref.phase_ref(11, b, n, 201)
        assert np.array_equal(ph[b, :n], ref) and not ph[b, n:].any()
        assert np.array_equal(ph4[b, :n], ref) and not ph4[b, n:].any()
    assert ph.min() >= 0.0 and ph.max() < np.float32(np.pi) and abs(ph[1, :1200].mean() - np.pi / 2) < 0.01
    alone = audio_lib.phase_init([999], 1000, 201, seed=11, utt_ids=[5]).cpu().numpy()              # another Fmax, alone
    assert np.array_equal(alone[0, :999], ph[5, :999])
    other = audio_lib.phase_init(nf, 1201, 201, seed=12).cpu().numpy()
    assert not np.array_equal(other[1], ph[1])
    big = audio_lib.phase_init([3], 3, 201, seed=(1 << 63) + 5, utt_ids=[-7]).cpu().numpy()         # all 64 seed bits, any id
    assert np.array_equal(big[0], philox_ref.phase_ref((1 << 63) + 5, -7, 3, 201))


def test_vocoder_takes_the_device_phase():
    import audio_lib
    rng = np.random.RandomState(2)
    P = rng.uniform(0.0, 0.9, (3, 500, 201)).astype(np.float32)
    nf = [500, 400, 123]
    kw = dict(P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80, win_length=400, mean_abs_amp_norm=0.045, n_iter=3)
    got = audio_lib.from_power_to_wav_batch(P, nf, phase0='device', seed=9, utt_ids=[4, 5, 6], **kw)
    ph = np.zeros((3, 500, 201), np.float32)
    for b in range(3):
        ph[b, :nf[b]] = philox_ref.phase_ref(9, 4 + b, nf[b], 201)
    want = audio_lib.from_power_to_wav_batch(P, nf, phase0=ph, **kw)
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match='phase0'):
        audio_lib.griffin_lim_batch(P, nf, phase0='host')


# --------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def f32_models(golden_dir):
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    enc_cfg, dec_cfg, c = _cfgs(golden_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(enc_cfg, None)
        dec = decoder_specs(dec_cfg, None, enc)
    wd = mo.init_weights(dec_cfg, 'decoder', seed=2, perturb_bn=True)
    dec.store.load_dict(dict(wd), strict=False)
    return dec, wd, enc_cfg, dec_cfg, c


def _ragged():
    lens = [int(s * 16000) for s in SECONDS]
    wav = np.zeros((len(lens), max(lens)), np.float32)
    for b, L in enumerate(lens):
        wav[b, :L] = fo.synth_speech(1, L, seed=11 + b)[0]
    return wav, lens


@pytest.fixture(scope='module')
def numpy_phase_run(f32_models):
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    np.random.seed(7)
    r = conversion.convert_batch(dec, wav, lens, c, t_s=0, t_e=60, n_iter=N_ITER, giffin_lim_input=True, phase='numpy')
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize('b', [0, 1, 2])
def test_ragged_batch_against_the_oracle_chain(golden_dir, f32_models, numpy_phase_run, b):
    """Utterance b of the ragged batch against the oracle chain, as test_config1_single_utterance_conversion does it for
    one utterance (same weights, same tolerances, same draw order: per utterance the true spectrum's phase, then the
    predicted one's)."""
    import tf_bundle
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    r = numpy_phase_run
    wav, lens = _ragged()
    L = lens[b]
    F = 1 + L // 80
    n_win = {0: 2, 1: 1, 2: 3}[b]
    n = 400 * n_win
    assert r.n_frames == [800, 400, 1200] and r.n_samples == [80 * 799, 80 * 399, 80 * 1199]
    assert r.mel_pred.shape == (3, 1200, 80) and r.stft_pred.shape == (3, 1200, 201) and r.phn_pred.shape == (3, 1200, 61)
    assert r.y_wav_pred.shape == r.y_wav_true.shape == (3, 80 * 1199) and r.y_wav_pred.is_cuda
    g = lambda t: t[b].cpu().numpy()
    mel_pred, stft_pred, phn_pred, mel_true, stft_true = (g(t) for t in (r.mel_pred, r.stft_pred, r.phn_pred, r.mel_true, r.stft_true))
    y_true, y_pred = g(r.y_wav_true), g(r.y_wav_pred)

    o_mfcc, o_mel, o_stft = fo.calc_MFCC_input(wav[b, :L], **_fe_kwargs(c))
    total, n_s, n_e = co.window_plan(F, 16000, 80, 400, 0, 60)
    assert (total, n_s, n_e) == (n, 0, n)
    pad = lambda a: np.concatenate([a, np.zeros((total - F, a.shape[1]))], 0)
    p_mfcc, p_stft, p_mel = pad(o_mfcc), pad(o_stft), pad(o_mel)
    enc_w = mo.to_torch(tf_bundle.read_bundle(os.path.join(golden_dir, 'enc_14_ckpt', 'encoder-136512')), torch.float64)
    dec_w = mo.to_torch(wd, torch.float64)
    y0 = _oracle_predict(p_mfcc[n_s:n_e].reshape(-1, 400, 80), enc_w, dec_w, enc_cfg, dec_cfg)
    if n_win > 1:
        y1 = _oracle_predict(p_mfcc[n_s + 200:n_e - 200].reshape(-1, 400, 80), enc_w, dec_w, enc_cfg, dec_cfg)
        o_mel_pred, o_stft_pred, o_phn = (co.compound(a, c_) for a, c_ in zip(y0, y1))
    else:
        o_mel_pred, o_stft_pred, o_phn = (a.reshape(-1, a.shape[-1]) for a in y0)

    # ---- integer contract: N*400 frames, zeros beyond; the true spectra are the padded front-end rows
    for a in (mel_pred, stft_pred, phn_pred, mel_true, stft_true):
        assert not a[n:].any()
    assert not y_true[80 * (n - 1):].any() and not y_pred[80 * (n - 1):].any()
    assert not stft_true[F:n].any() and not mel_true[F:n].any()
    assert np.abs(mel_true[:F] - o_mel).max() < 1e-4 and np.abs(stft_true[:F] - o_stft).max() < 2e-4
    # ---- floating-point parity
    e = dict(phn=np.abs(phn_pred[:n] - o_phn).max(), mel=np.abs(mel_pred[:n] - o_mel_pred).max(),
             stft=np.abs(stft_pred[:n] - o_stft_pred).max())
    print('utterance %d: max |err| vs oracle: %s' % (b, e))
    assert e['phn'] < 5e-4 and e['mel'] < 1e-3 and e['stft'] < 1e-3

    # ---- audio: the generator's state at utterance b is that of a loop of conversion2 calls over the batch
    rs = np.random.RandomState(7)
    for k in range(b):
        rs.rand(201, r.n_frames[k]); rs.rand(201, r.n_frames[k])
    kw = dict(P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80, win_length=400,
              mean_abs_amp_norm=15 * 0.003, n_iter=N_ITER, n_fft=None)
    o_true = vo.from_power_to_wav(p_stft[n_s:n_e], realse=1.0, phase0=np.pi * rs.rand(201, n), **kw)
    ph_pred = np.pi * rs.rand(201, n)
    yt, yp = y_true[:80 * (n - 1)], y_pred[:80 * (n - 1)]
    assert np.isfinite(yp).all()
    assert abs(np.abs(yt).mean() - 0.045) < 1e-5 and abs(np.abs(yp).mean() - 0.045) < 1e-5
    et = np.abs(yt - o_true).max() / np.abs(o_true).max()
    o_pred = vo.from_power_to_wav(stft_pred[:n], realse=1.0, phase0=ph_pred, **kw)
    ep = np.abs(yp - o_pred).max() / np.abs(o_pred).max()
    print('utterance %d: waveform err / peak: true %.3e pred %.3e' % (b, et, ep))
    assert et < 1e-2 and ep < 1e-3


def test_numpy_phase_matches_a_loop_of_conversion2(f32_models, numpy_phase_run):
    """Draw for draw: the batch under np.random.seed(7) equals conversion2 called per utterance under the same seed
    (features from the same batched front-end call)."""
    import audio_lib
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    np.random.seed(7)
    for b, L in enumerate(lens):
        mfcc, mel, stft = audio_lib.calc_MFCC_input(wav[b, :L], **_fe_kwargs(c))
        with contextlib.redirect_stdout(io.StringIO()):
            r1 = conversion.conversion2(dec, mfcc, mel, stft, c, t_s=0, t_e=60, n_iter=N_ITER)
        n = numpy_phase_run.n_frames[b]
        got = numpy_phase_run.y_wav_pred[b, :80 * (n - 1)].cpu().numpy()
        assert np.abs(numpy_phase_run.stft_pred[b, :n].cpu().numpy() - r1.stft_pred).max() < 1e-3
        assert np.abs(got - r1.y_wav_pred).max() < 1e-3 * np.abs(r1.y_wav_pred).max()
        gt = numpy_phase_run.y_wav_true[b, :80 * (n - 1)].cpu().numpy()
        assert np.abs(gt - r1.y_wav_true).max() < 1e-3 * np.abs(r1.y_wav_true).max()


def test_device_phase_through_convert_batch(f32_models):
    import audio_lib
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_batch(dec, wav, lens, c, n_iter=N_ITER, phase='device', seed=5)
    assert r.y_wav_true is None
    ph = np.zeros((3, 1200, 201), np.float32)
    for b in range(3):
        ph[b, :r.n_frames[b]] = philox_ref.phase_ref(5, b, r.n_frames[b], 201)
    want = audio_lib.from_power_to_wav_batch(r.stft_pred, r.n_frames, P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80,
                                             win_length=400, mean_abs_amp_norm=15 * 0.003, n_iter=N_ITER, phase0=ph)
    assert torch.equal(r.y_wav_pred, want)
    # utterance 2 alone, under its own id: same phase (phase_ref above does not know the batch), waveform within the
    # waveform tolerance of its row in the batch (the decoder's summation order may depend on the batch)
    one = conversion.convert_batch(dec, wav[2:3], lens[2:3], c, n_iter=N_ITER, phase='device', seed=5, utt_ids=[2])
    assert one.n_frames == [1200]
    a, bt = one.y_wav_pred[0].cpu().numpy(), r.y_wav_pred[2].cpu().numpy()
    assert np.abs(a - bt).max() < 1e-3 * np.abs(bt).max()
    assert np.abs(one.stft_pred[0].cpu().numpy() - r.stft_pred[2].cpu().numpy()).max() < 1e-3
    other = conversion.convert_batch(dec, wav[2:3], lens[2:3], c, n_iter=N_ITER, phase='device', seed=5, utt_ids=[3])
    assert not torch.equal(other.y_wav_pred, one.y_wav_pred)
    # realse != 1 and the single-pass form run through the same call
    r2 = conversion.convert_batch(dec, wav, lens, c, n_iter=N_ITER, seed=5, realse=1.2, two_pass=False)
    assert torch.isfinite(r2.y_wav_pred).all() and not torch.equal(r2.y_wav_pred, r.y_wav_pred)
    assert (r2.stft_pred[1] - r.stft_pred[1]).abs().max() < 1e-3   # one window: both forms are the reshape
    # a phase given as a tensor
    r3 = conversion.convert_batch(dec, wav, lens, c, n_iter=N_ITER, phase=ph)
    assert torch.equal(r3.y_wav_pred, r.y_wav_pred)
    r4 = conversion.convert_batch(dec, wav, lens, c, vocode=False)
    assert r4.y_wav_pred is None and torch.equal(r4.stft_pred, r.stft_pred)


def test_no_host_synchronisation_inside_the_call(f32_models):
    """cuda inputs, warmed up: under torch's sync debug mode 'error' any device-to-host copy, blocking upload or host
    wait inside convert_batch raises.  The probe first shows that the mode does raise on this build."""
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    d_wav = _dev(wav)
    conversion.convert_batch(dec, d_wav, lens, c, n_iter=N_ITER, giffin_lim_input=True, window_batch=4)     # warm-up
    torch.cuda.synchronize()
    one = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            one.item()                                           # the mode works: a host read of device data is an error
        r = conversion.convert_batch(dec, d_wav, lens, c, n_iter=N_ITER, giffin_lim_input=True, window_batch=4)
        rn = conversion.convert_batch(dec, d_wav, lens, c, n_iter=N_ITER, phase='numpy', momentum=0.5)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(r.y_wav_pred).all() and torch.isfinite(rn.y_wav_pred).all() and torch.isfinite(r.y_wav_true).all()


def test_momentum_through_convert_batch(f32_models):
    """momentum 0.99, 32 iterations through convert_batch: finite; bit-identical to from_power_to_wav_batch on its own
    stft_pred from the reference phase, whose trace is finite; and on those magnitudes the convergence check of
    test_vocoder_momentum_gpu.py holds: spectral convergence within 2 % of the float64 reference's from the same
    phase, and no worse than 1.1 x that of 200 plain iterations."""
    import _vc
    import audio_lib
    import conversion
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    r = conversion.convert_batch(dec, wav[:1, :lens[0]], lens[:1], c, n_iter=32, momentum=0.99, phase='device', seed=3)
    assert torch.isfinite(r.y_wav_pred).all() and r.n_frames == [800]
    ph = philox_ref.phase_ref(3, 0, 800, 201)
    want, tr = audio_lib.from_power_to_wav_batch(r.stft_pred, [800], P_dB_norm_factor=0.01, pre_emphasis=0.97, hop_length=80,
                                                 win_length=400, mean_abs_amp_norm=15 * 0.003, n_iter=32, phase0=ph[None],
                                                 momentum=0.99, trace=True)
    assert torch.equal(r.y_wav_pred, want)
    tr = tr.cpu().numpy()[1:, 0]
    assert np.isfinite(tr).all() and (tr > 0).all() and tr[-1] < tr[0]
    amp = torch.empty_like(r.stft_pred)
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(r.stft_pred), None, 1, 800, 201, 0.01, 1.0, _vc.ptr(amp), _vc.current_stream()))
    a64 = amp[0].cpu().numpy().astype(np.float64).T                                               # [bins, F]
    sc = {}
    for m, n in ((0.0, 200), (0.99, 32)):
        y = audio_lib.griffin_lim_batch(amp, None, 400, 80, num_iters=n, phase0=ph[None], momentum=m)[0].cpu().numpy()
        sc[(m, n)] = fr.sc(y, a64, 400, 80)
    ref = fr.sc(fr.griffin_lim_momentum(a64, 400, 80, 32, 0.99, phase0=ph.T.astype(np.float64)), a64, 400, 80)
    print('spectral convergence: device %s, float64 reference (0.99, 32) %.5f' % (sc, ref))
    assert abs(sc[(0.99, 32)] - ref) <= 0.02 * ref
    assert sc[(0.99, 32)] <= 1.1 * sc[(0.0, 200)]


@pytest.mark.parametrize('kind', ['bfloat16', 'mxfp8'])
def test_low_precision_decoders_through_convert_batch(golden_dir, f32_models, kind):
    """bf16 models, and an MX-FP8 decoder (built without an encoder: it owns its store) fed by the bf16 encoder: runs,
    finite, mel_pred / stft_pred within the end-to-end bound (B) of test_bench_config_gpu.py (max <= 0.25 max(1, |ref|max),
    rms <= 5e-2 max(1, |ref| rms): dominated by the bf16 encoder's argmax flips), for MX-FP8 plus the derived decoder
    bound (D) of test_mx8_gpu.py (max 3.0e-2, rms 7e-3).  Reference: the float32 models on the same batch, which the
    tests above hold within 1e-3 of the float64 oracle -- far inside both bounds."""
    import conversion
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    dec32, wd, enc_cfg, dec_cfg, c = f32_models
    enc_cfg = dict(enc_cfg, compute_dtype='bfloat16')
    dec_cfg = dict(dec_cfg, compute_dtype=kind)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = encoder_spec_phn(enc_cfg, None)
        dec = decoder_specs(dec_cfg, None, enc if kind == 'bfloat16' else None)
        if kind == 'mxfp8':
            enc.restore()
    dec.store.load_dict(dict(wd), strict=False)
    wav, lens = _ragged()
    ref = conversion.convert_batch(dec32, wav, lens, c, vocode=False)
    r = conversion.convert_batch(dec, wav, lens, c, n_iter=N_ITER, seed=1, encoder=enc if kind == 'mxfp8' else None)
    assert torch.isfinite(r.y_wav_pred).all() and float(r.y_wav_pred.abs().max()) > 0
    assert r.phn_pred.shape == (3, 1200, 61) and torch.isfinite(r.phn_pred).all()
    add_max, add_rms = (3.0e-2, 7e-3) if kind == 'mxfp8' else (0.0, 0.0)
    for name in ('mel_pred', 'stft_pred'):
        d, f = getattr(r, name).cpu().numpy().astype(np.float64), getattr(ref, name).cpu().numpy().astype(np.float64)
        err = np.abs(d - f)
        s = dict(max=err.max(), rms=np.sqrt((err ** 2).mean()), ref_max=np.abs(f).max(), ref_rms=np.sqrt((f ** 2).mean()))
        print(kind, name, s)
        assert s['max'] <= 0.25 * max(1.0, s['ref_max']) + add_max, (name, s)
        assert s['rms'] <= 5e-2 * max(1.0, s['ref_rms']) + add_rms, (name, s)


# --------------------------------------------------------------------------------------------- graph replay
def test_graph_replay_of_the_three_launches():
    """In the manner of test_graph_replay_gpu.py: warm-up, capture one stream, replay with NEW inputs copied into the
    static tensors (data, tables and frame counts), each replay bit-identical to eager calls on the same inputs."""
    import audio_lib
    import conversion
    from test_graph_replay_gpu import _capture, _free, _same
    frames_k = ([300, 799, 1001, 2000], [2000, 300, 799, 1001], [799, 1001, 2000, 300])
    plans = [_plan(f) for f in frames_k]
    assert len({p.W for p in plans}) == 1 and len({p.Fout for p in plans}) == 1
    p0 = plans[0]
    Fmax = 2003
    s_src = torch.zeros((4, Fmax, 201), device='cuda')
    s_win, s_utt, s_clip, s_nout = _dev(p0.win_tab), _dev(p0.utt_tab), _dev(p0.n_clip), _dev(p0.n_out)
    s_ids = _dev(np.arange(4, dtype=np.int32))

    def chain(src, win, utt, clip, nout, ids):
        x = conversion.cut_windows(src, win, clip, 400)
        P, amp = conversion.compound_stitch(x, utt, p0.Fout, P_dB_norm_factor=0.01)
        ph = audio_lib.phase_init(nout, p0.Fout, 201, seed=3, utt_ids=ids)
        return x, P, amp, ph

    g, outs = _capture(lambda: chain(s_src, s_win, s_utt, s_clip, s_nout, s_ids))
    try:
        for k, p in enumerate(plans):
            src = _dev(np.random.RandomState(40 + k).uniform(-0.2, 0.9, (4, Fmax, 201)).astype(np.float32))
            tabs = [_dev(p.win_tab), _dev(p.utt_tab), _dev(p.n_clip), _dev(p.n_out), _dev(np.arange(4, dtype=np.int32) + 10 * k)]
            s_src.copy_(src)
            for s, t in zip((s_win, s_utt, s_clip, s_nout, s_ids), tabs):
                s.copy_(t)
            g.replay()
            torch.cuda.synchronize()
            want = chain(src, *tabs)
            for name, a, b in zip(('windows', 'stitched', 'amp', 'phase'), outs, want):
                _same(a, b, 'replay %d %s' % (k, name))
            assert float(outs[3][0, :int(p.n_out[0])].max()) > 3.0
    finally:
        _free(g)
