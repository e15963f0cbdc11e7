"""The harmonic-plus-noise vocoder on the device (csrc/vc_hnm.hip): every launch alone against tests/hnm_ref.py on the device's
own inputs -- the plan and the noise bit for bit, the envelope, the noise gain and the synthesis within the float32 model's
bound -- then graph replay of the whole chain and three behaviours of audio_lib.hnm_synth_batch on one second of audio or
less: the envelope read back from the waveform, the pitch read back by YIN, and the level of the noise branch.

The synthesis kernel's tile is vc_hnm_tile_intervals() = 16 intervals: F = 33 puts intervals on both sides of a tile border,
F = 2 is one interval.  The envelope kernel takes 8 frames per workgroup at these sizes; F = 5 with n_frames [5, 1, 0] has a
partly live tile; the chain and behaviour tests (F = 19 to 201) run several tiles."""
import numpy as np
import pytest
import torch

import hnm_ref as R
from test_convert_batch_gpu import _ragged, f32_models      # noqa: F401  (f32_models: a module-scoped fixture)
from test_hnm_cpu import ROUND_TRIP_F, ROUND_TRIP_RMS

pytestmark = pytest.mark.gpu

SR, HOP = 16000, 80
POISON = 0x7FC00000                     # a NaN's bits: what an unwritten output would still hold


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _poison(shape, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full(shape, 0xAB, dtype=dtype, device='cuda')
    return torch.full(shape, POISON, dtype=torch.int32, device='cuda').view(dtype)


def run_envelope(amp, n_frames, n_fft, order, iters, floor=1e-5):
    import _vc
    import audio_lib
    B, F, nb = amp.shape
    d_amp, d_nf = _dev(amp), None if n_frames is None else _dev(np.asarray(n_frames, np.int32))
    out = _poison((2, B, F, nb))
    _vc.check(_vc.lib().vc_env_cepstral_f32(_vc.ptr(d_amp), _vc.ptr(d_nf), _vc.ptr(audio_lib._env_table(n_fft)), B, F, n_fft, order,
                                            iters, floor, _vc.ptr(out[0]), _vc.ptr(out[1]), _vc.current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(d_amp.cpu().numpy().view(np.int32), amp.view(np.int32))
    out = out.cpu().numpy()
    return out[0], out[1]


def check_envelope(amp, n_frames, n_fft, order, iters, need_margin):
    """Device against reference within the model's bound, zeros beyond n_frames; returns the worst fraction of the bound."""
    env, th = run_envelope(amp, n_frames, n_fft, order, iters)
    worst = 0.0
    for b in range(amp.shape[0]):
        n = amp.shape[1] if n_frames is None else n_frames[b]
        assert not env[b, n:].any() and not th[b, n:].any()
        if n == 0:
            continue
        E, T, bE, bT, margin = R.envelope(amp[b, :n], n_fft, order, iters, 1e-5)
        if need_margin:
            assert margin > 1.0, margin                             # the device took the reference's branch at every max step
        for got, want, bound in ((env[b, :n], E, bE), (th[b, :n], T, bT)):
            err = np.abs(got - want)
            assert (err <= bound).all(), (n_fft, order, iters, float((err - bound).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))    # (theta's bound is 0 at bin 0: sin 0)
    return worst


@pytest.mark.parametrize('n_fft', [16, 400])
def test_envelope_against_reference(n_fft):
    """General random spectra, order in {1, 24 (3 at n_fft 16), N/2 - 1}, iters in {0, 1, 16}, B = 3 with n_frames [F, 1, 0].
    With iters <= 1 the data's margins |a - E| exceed the bound at every max step (checked on the reference), so the device
    provably took the reference's branch.  With 16 iterations the true envelope converges ONTO the peaks of the data -- the
    margins shrink to nothing by design -- and the bound holds through the max step by its Lipschitz constant instead
    (hnm_ref.envelope).  The worst fraction of the bound is printed (profiles/hnm/test_hnm_gpu.log)."""
    nb = n_fft // 2 + 1
    rng = np.random.default_rng(1)
    for order in (1, 24 if n_fft == 400 else 3, n_fft // 2 - 1):
        for iters in (0, 1, 16):
            amp = np.exp(rng.normal(0.0, 1.5, (3, 5, nb))).astype(np.float32)
            worst = check_envelope(amp, [5, 1, 0], n_fft, order, iters, need_margin=iters <= 1)
            print('envelope n_fft %d order %d iters %d: worst fraction of the bound %.4f' % (n_fft, order, iters, worst))


@pytest.mark.parametrize('n_fft', [16, 400])
def test_envelope_identities(n_fft):
    nb = n_fft // 2 + 1
    rng = np.random.default_rng(2)
    # a constant spectrum: env_log = log c, theta = 0
    amp = np.full((1, 5, nb), 0.25, np.float32)
    env, th = run_envelope(amp, None, n_fft, min(24, n_fft // 2 - 1), 3)
    bE, bT = R.envelope(amp[0], n_fft, min(24, n_fft // 2 - 1), 3, 1e-5)[2:4]
    assert (np.abs(env[0] - np.log(0.25)) <= bE).all() and (np.abs(th[0]) <= bT).all()
    # order N/2 - 1, iters 0 reproduces log(max(amp, floor)) -- for data without the one coefficient that order leaves out,
    # c_{N/2} = sum_k w_k (-1)^k a_k / N (what rounding amp to float32 puts back is below 1e-6)
    a = rng.normal(0.0, 1.0, (1, 5, nb))
    w = np.full(nb, 2.0)
    w[0] = w[-1] = 1.0
    alt = (-1.0) ** np.arange(nb)
    a -= ((a * w * alt).sum(axis=2) / n_fft)[:, :, None] * alt
    amp = np.exp(a).astype(np.float32)
    want = np.log(amp.astype(np.float64))
    env, _ = run_envelope(amp, None, n_fft, n_fft // 2 - 1, 0)
    E, _, bE, _, _ = R.envelope(amp[0], n_fft, n_fft // 2 - 1, 0, 1e-5)
    assert np.abs(E - want[0]).max() < 1e-6                         # the data is what it was built to be
    assert (np.abs(env[0] - want[0]) <= bE + 1e-6).all()
    # the floor: magnitudes below it, zero included, count as the floor itself
    low = amp.copy()
    low[0, :, 3] = 0.0
    low[0, :, 5] = 1e-4
    at = low.copy()
    at[0, :, 3] = at[0, :, 5] = 1e-3
    got, ref = run_envelope(low, None, n_fft, 3, 2, floor=1e-3), run_envelope(at, None, n_fft, 3, 2, floor=1e-3)
    assert np.array_equal(got[0].view(np.int32), ref[0].view(np.int32)) and np.array_equal(got[1].view(np.int32), ref[1].view(np.int32))


# ------------------------------------------------------------------------------------------ plan
def run_plan(f0, n_frames, hop, f0_lo=40.0, f0_hi=SR / 4.0, sr=SR):
    import _vc
    B, F = f0.shape
    d_f0, d_nf = _dev(f0), None if n_frames is None else _dev(np.asarray(n_frames, np.int32))
    voiced = _poison((B, F), torch.uint8)
    tab = _poison((3, B, F), torch.int32)
    flags = _poison((B,), torch.int32)
    _vc.check(_vc.lib().vc_hnm_plan(_vc.ptr(d_f0), _vc.ptr(d_nf), B, F, sr, hop, f0_lo, f0_hi, _vc.ptr(voiced), _vc.ptr(tab[0]),
                                    _vc.ptr(tab[1]), _vc.ptr(tab[2]), _vc.ptr(flags), _vc.current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(d_f0.cpu().numpy().view(np.int32), f0.view(np.int32))
    tab = tab.cpu().numpy()
    return dict(voiced=voiced.cpu().numpy(), inc=tab[0].view(np.uint32), slope=tab[1], phase=tab[2].view(np.uint32),
                flags=flags.cpu().numpy())


def check_plan(got, f0, n_frames, hop, **kw):
    for b in range(len(f0)):
        want = R.plan(f0[b], f0.shape[1] if n_frames is None else n_frames[b], kw.get('sr', SR), hop, kw.get('f0_lo', 40.0),
                      kw.get('f0_hi', SR / 4.0))
        for k in ('voiced', 'inc', 'slope', 'phase'):
            assert np.array_equal(got[k][b], want[k]), (b, k)
        assert got['flags'][b] == want['flags'], b


def plan_rows(F, rng):
    """Voiced and unvoiced runs at both ends and in the middle; all unvoiced; one voiced frame; the limits, just outside them,
    NaN, negative and infinite values."""
    rows = np.zeros((6, F), np.float32)
    rows[0] = rng.uniform(60.0, 900.0, F)
    rows[0, :3] = rows[0, 10:14] = rows[0, F - 5:] = 0.0
    rows[2, F // 2] = 123.0
    rows[3] = rng.uniform(60.0, 900.0, F)
    rows[3, :8] = [40.0, 4000.0, np.nextafter(np.float32(40), np.float32(0)), np.nextafter(np.float32(4000), np.float32(1e9)),
                   np.nan, -100.0, np.inf, 0.0]
    rows[4] = rng.uniform(3000.0, 4000.0, F)                        # voiced from the first frame to the last
    rows[5, F - 1] = 77.0                                           # a leading run that is the whole row but one
    return rows


@pytest.mark.parametrize('hop', [1, 80, 256])
def test_plan_bit_for_bit(hop):
    rng = np.random.default_rng(10 + hop)
    F = 300                                                         # two tiles of 256 frames
    f0 = plan_rows(F, rng)
    n_frames = [F, F, F, F, 257, F]
    got = run_plan(f0, n_frames, hop)
    check_plan(got, f0, n_frames, hop)
    assert got['flags'].tolist() == [0, 0, 0, 1, 0, 0]
    for b in (0, 3, 4):                                             # the same rows alone give the same bits
        one = run_plan(f0[b:b + 1], n_frames[b:b + 1], hop)
        for k in one:
            assert np.array_equal(one[k][0], got[k][b]), (b, k)
    for n in ([0, 1, 2, 255, 256, F - 1],):
        check_plan(run_plan(f0, n, hop), f0, n, hop)
    check_plan(run_plan(f0, None, hop), f0, None, hop)


def test_plan_long_utterance_wraps_the_phase():
    """F = 16,384 with f0 near sr / 4: the phase wraps about 20 times a frame at hop 80, 300,000 times in all."""
    rng = np.random.default_rng(4)
    F = 16384
    f0 = rng.uniform(3500.0, 4000.0, (2, F)).astype(np.float32)
    f0[1, rng.random(F) < 0.4] = 0.0
    for hop in (80, 256):
        got = run_plan(f0, [F, F - 7], hop)
        check_plan(got, f0, [F, F - 7], hop)
        assert len(np.unique(got['phase'][0] >> 28)) == 16


# ------------------------------------------------------------------------------------------ noise
def test_noise_bit_for_bit():
    import audio_lib
    lens = [1000, 0, 37, 1 << 16]
    ids = [5, 6, 7, 3]
    x = audio_lib.noise_batch(lens, 1 << 16, seed=7, utt_ids=ids).cpu().numpy()
    for b, (n, i) in enumerate(zip(lens, ids)):
        assert np.array_equal(x[b, :n].view(np.int32), R.noise(7, i, n).view(np.int32)) and not x[b, n:].any()
    # independent of the place in the batch and of Lmax; the default ids are the row numbers
    y = audio_lib.noise_batch([37, 1001], 1001, seed=7, utt_ids=torch.tensor([7, 5], dtype=torch.int32, device='cuda')).cpu().numpy()
    assert np.array_equal(y[0, :37], x[2, :37]) and np.array_equal(y[1, :1000], x[0, :1000])
    z = audio_lib.noise_batch(torch.tensor([9, 9], dtype=torch.int32, device='cuda'), 9, seed=2 ** 64 - 1).cpu().numpy()
    assert np.array_equal(z[1], R.noise(2 ** 64 - 1, 1, 9)) and np.array_equal(z[0], R.noise(2 ** 64 - 1, 0, 9))
    # mean and variance of 2^16 samples: the figures of test_hnm_cpu.test_noise_reference_statistics
    v = x[3].astype(np.float64)
    assert abs(v.mean()) < 4 * 2.0 ** -8 and abs(v.var() - 1.0) < 4 * np.sqrt(0.8 / 65536)


def test_noise_gain():
    import _vc
    rng = np.random.default_rng(6)
    B, F, nb, cut = 3, 7, 201, 100
    env = rng.uniform(-11.0, 3.0, (B, F, nb)).astype(np.float32)
    voiced = (rng.random((B, F)) < 0.5).astype(np.uint8)
    n_frames = [F, 3, 0]
    gscale = np.float32(0.7 / np.sqrt(150.0))
    G = _poison((B, F, nb))
    d = [_dev(env), _dev(voiced), _dev(np.asarray(n_frames, np.int32))]
    _vc.check(_vc.lib().vc_hnm_noise_gain_f32(_vc.ptr(d[0]), _vc.ptr(d[1]), _vc.ptr(d[2]), B, F, nb, cut, float(gscale), _vc.ptr(G),
                                              _vc.current_stream()))
    G = G.cpu().numpy()
    for b in range(B):
        want, rel = R.noise_gain(env[b], voiced[b], n_frames[b], cut, gscale)
        assert (np.abs(G[b] - want) <= rel * want).all()
        assert not G[b][want == 0].any() and not G[b, n_frames[b]:].any()
        assert not G[b, :n_frames[b]][voiced[b, :n_frames[b]] == 1][:, :cut].any()


# ------------------------------------------------------------------------------------------ synthesis
def run_synth(env, th, pl, n_frames, n_fft, hop, cutoff_inc, scale, add=None):
    import _vc
    B, F, _ = env.shape
    d = [_dev(env), _dev(th), _dev(pl['voiced']), _dev(pl['inc'].view(np.int32)), _dev(pl['slope']), _dev(pl['phase'].view(np.int32))]
    d_nf = None if n_frames is None else _dev(np.asarray(n_frames, np.int32))
    d_add = None if add is None else _dev(add)
    y = _poison((B, hop * (F - 1)))
    _vc.check(_vc.lib().vc_hnm_synth_f32(*[_vc.ptr(t) for t in d], _vc.ptr(d_nf), _vc.ptr(d_add), B, F, n_fft, hop, cutoff_inc,
                                         float(scale), _vc.ptr(y), _vc.current_stream()))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def smooth_rows(rng, B, F, nb, lo=-9.0, hi=-2.0):
    """(env_log, theta) float32 [B, F, nb]: smooth in frequency, different from frame to frame."""
    k = np.linspace(0.0, 1.0, nb)
    e = rng.uniform(lo, hi, (B, F, 1)) + rng.uniform(0.5, 2.0, (B, F, 1)) * np.cos(2.0 * np.pi * rng.uniform(1.0, 4.0, (B, F, 1)) * k)
    t = rng.uniform(-1.5, 1.5, (B, F, 1)) * np.sin(2.0 * np.pi * rng.uniform(1.0, 3.0, (B, F, 1)) * k)
    return e.astype(np.float32), t.astype(np.float32)


def check_synth(f0, n_frames, n_fft, hop, cutoff_hz, f0_lo, with_add, seed):
    rng = np.random.default_rng(seed)
    B, F = f0.shape
    nb = n_fft // 2 + 1
    env, th = smooth_rows(rng, B, F, nb)
    pl = run_plan(f0, n_frames, hop, f0_lo=f0_lo)
    check_plan(pl, f0, n_frames, hop, f0_lo=f0_lo)
    cut = max(1, min(int(round(cutoff_hz * 2.0 ** 32 / SR)), 2 ** 31))
    scale = np.float32(2.0 / R.window(n_fft, n_fft).sum())
    add = rng.normal(0.0, 0.01, (B, hop * (F - 1))).astype(np.float32) if with_add else None
    y = run_synth(env, th, pl, n_frames, n_fft, hop, cut, scale, add)
    worst, kmax = 0.0, 0
    for b in range(B):
        one = {k: v[b] for k, v in pl.items()}
        n = F if n_frames is None else n_frames[b]
        want, bound = R.synth(env[b], th[b], one, n, n_fft, hop, cut, scale, None if add is None else add[b])
        live = hop * max(n - 1, 0)
        assert not y[b, live:].any()
        err = np.abs(y[b] - want)
        assert (err <= bound).all(), (b, float((err / np.maximum(bound, 1e-30)).max()))
        if bound.max() > 0:
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        inc = one['inc'].astype(np.int64)
        kmax = max(kmax, int(np.where(one['voiced'] != 0, (cut - 1) // np.maximum(inc, 1), 0)[:max(n, 0)].max(initial=0)))
    return worst, kmax, np.abs(y).max()


def test_synth_against_reference():
    """A glide across the cutoff (the harmonic count changes between an interval's ends), onsets and offsets, a tile seam
    (F = 33: intervals 15 | 16), ragged rows, F = 2, and f0 = f0_lo with the cutoff at Nyquist (K near the cap of 256)."""
    F = 33
    t = np.arange(F)
    glide = (300.0 + 250.0 * t / (F - 1)).astype(np.float32)        # 2 kHz / f0: 6 harmonics down to 3
    gaps = glide.copy()
    gaps[:2] = gaps[9:12] = gaps[15:18] = gaps[F - 3:] = 0.0        # onset, offsets, and both across the tile border
    vib = (120.0 * (1.0 + 0.1 * np.sin(2.0 * np.pi * 5.0 * t * HOP / SR))).astype(np.float32)
    f0 = np.stack([glide, gaps, vib])
    for n_frames, add in ((None, False), ([F, 18, 1], True)):
        worst, kmax, peak = check_synth(f0, n_frames, 400, HOP, 2000.0, 40.0, add, 21)
        print('synthesis glide / gaps / vibrato, add %s: worst fraction of the bound %.4f, peak %.3g' % (add, worst, peak))
        assert peak > 1e-3
    worst, kmax, _ = check_synth(f0[:, :2].copy(), None, 400, HOP, 4000.0, 40.0, True, 22)
    print('synthesis F = 2: worst fraction of the bound %.4f' % worst)
    low = np.full((1, F), 32.0, np.float32)
    low[0, 20:] = 33.5
    worst, kmax, _ = check_synth(low, None, 400, HOP, 8000.0, 32.0, False, 23)
    print('synthesis f0 = f0_lo = 32 Hz, cutoff at Nyquist: %d harmonics, worst fraction of the bound %.4f' % (kmax, worst))
    assert 240 <= kmax <= 256
    worst, _, _ = check_synth(f0[:2, :9].copy(), [9, 4], 16, 3, 3000.0, 40.0, True, 24)
    print('synthesis n_fft 16, hop 3: worst fraction of the bound %.4f' % worst)


def test_synth_exact_properties():
    rng = np.random.default_rng(8)
    F, nb = 9, 201
    scale = np.float32(2.0 / R.window(400, 400).sum())
    cut = 1 << 30
    # 250 Hz at 16 kHz is inc = 2^26: with a frame-constant envelope the waveform repeats every 64 samples bit for bit
    f0 = np.full((1, F), 250.0, np.float32)
    pl = run_plan(f0, None, HOP)
    assert (pl['inc'] == 1 << 26).all()
    env, th = smooth_rows(rng, 1, 1, nb, -2.0, 0.0)
    env, th = np.repeat(env, F, axis=1), np.repeat(th, F, axis=1)
    y = run_synth(env, th, pl, None, 400, HOP, cut, scale)[0]
    assert np.abs(y).max() > 1e-3
    assert np.array_equal(y[64:].view(np.int32), y[:-64].view(np.int32))
    # all unvoiced: exactly zero without add, add itself with it (its negative zeros included)
    env, th = smooth_rows(rng, 2, F, nb)
    pl = run_plan(np.zeros((2, F), np.float32), None, HOP)
    y = run_synth(env, th, pl, None, 400, HOP, cut, scale)
    assert np.array_equal(y.view(np.int32), np.zeros_like(y).view(np.int32))
    add = rng.normal(0.0, 1.0, y.shape).astype(np.float32)
    add[:, ::7] = -0.0
    y = run_synth(env, th, pl, None, 400, HOP, cut, scale, add)
    assert np.array_equal(y.view(np.int32), add.view(np.int32))


# ------------------------------------------------------------------------------------------ the chain
def vowel_batch(F, hz=(120.0, 200.0)):
    cases = [R.vowel(h, F) for h in hz]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases]


def test_chain_graph_replay():
    """Every launch of hnm_synth_batch, noise branch included, captured once and replayed twice: bit-identical to the eager
    run, and alone equals in the batch."""
    import audio_lib
    F = 19
    amp, f0, _ = vowel_batch(F)
    f0[1, 5:9] = 0.0
    d_amp, d_f0 = _dev(amp), _dev(f0)
    d_nf = torch.tensor([F, 12], dtype=torch.int32, device='cuda')
    eager = audio_lib.hnm_synth_batch(d_amp, d_f0, d_nf, seed=3)
    torch.cuda.synchronize()
    plan = audio_lib._get_voc_plan(400, HOP, 400)

    def launches():
        d_lens = (d_nf - 1).clamp_(min=0).mul_(HOP)
        return audio_lib._hnm_chain(plan, d_amp, d_f0, d_nf, d_lens, SR, 24, 16, 1e-5, 40.0, SR / 4.0,
                                    audio_lib.hnm_cutoff(4000.0, SR, 400, 40.0), 1.0, 3, None, True)

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = launches()
    for _ in range(2):
        out.y.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        for a, b in ((out.y, eager.y), (out.env_log, eager.env_log), (out.theta, eager.theta), (out.gain, eager.gain),
                     (out.plan.phase, eager.plan.phase), (out.plan.inc, eager.plan.inc)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    y = eager.y.cpu().numpy()
    assert np.abs(y[0]).max() > 1e-3 and not y[1, HOP * 11:].any() and np.abs(y[1, :HOP * 11]).max() > 1e-3
    one = audio_lib.hnm_synth_batch(d_amp[1:], d_f0[1:], [12], seed=3, utt_ids=[1])
    assert torch.equal(one.y[0].view(torch.int32), eager.y[1].view(torch.int32))


def test_round_trip_envelope():
    """The vowel through hnm_synth_batch(noise=False); the STFT of the DEVICE's waveform through envelope_batch comes back
    to the input envelope over the bins between 1.2 f0 and 7.4 kHz.  Cap: 1.5 x the rms the float64 reference gives on the
    same case (test_hnm_cpu.ROUND_TRIP_RMS: 0.851 dB at 120 Hz, 1.914 dB at 200 Hz)."""
    import audio_lib
    F = ROUND_TRIP_F
    amp, f0, envs = vowel_batch(F)
    out = audio_lib.hnm_synth_batch(amp, f0, noise=False, voiced_cutoff_hz=8000.0)
    y = out.y.cpu().numpy()
    estimate = lambda S: audio_lib.envelope_batch(S[None])[0][0].cpu().numpy()
    for b, hz in enumerate((120.0, 200.0)):
        rms, mean = R.round_trip_db(y[b], envs[b], hz, estimate=estimate)
        ref = R.round_trip_db(R.chain(amp[b], f0[b])[0], envs[b], hz)[0]
        print('round trip at %g Hz: device rms %.3f dB (mean %.3f), reference %.3f dB' % (hz, rms, mean, ref))
        assert abs(ref - ROUND_TRIP_RMS[hz]) < 0.01
        assert rms <= 1.5 * ROUND_TRIP_RMS[hz]


def _cents(f0_est, f0_true, sel):
    return float(np.abs(1200.0 * np.log2(f0_est[sel] / f0_true[sel])).mean())


def test_pitch_read_back():
    """evaluation.f0_batch (YIN) on the output against the contour asked for, on the fully voiced interior frames as the
    pitch tests select them (f0_ref.fully_voiced_frames) that YIN calls voiced on both waveforms.  Cap: the larger of 5 cents
    and twice the figure of the float64 reference waveform under the same tracker."""
    import evaluation as ev
    import f0_ref
    import audio_lib
    F = 51
    amp, f0, _ = vowel_batch(F)
    out = audio_lib.hnm_synth_batch(amp, f0, noise=False)
    ref = np.stack([R.chain(amp[b], f0[b], cutoff_hz=4000.0)[0] for b in range(2)]).astype(np.float32)
    got = ev.f0_batch(out.y, sr=SR, hop_length=HOP).f0.cpu().numpy()
    want = ev.f0_batch(ref, sr=SR, hop_length=HOP).f0.cpu().numpy()
    for b, hz in enumerate((120.0, 200.0)):
        sel = f0_ref.fully_voiced_frames(np.ones(HOP * (F - 1), bool), HOP, 512, f0_ref.lag_range(SR)[1])[:F]
        sel &= (got[b, :F] > 0) & (want[b, :F] > 0)
        assert sel.sum() >= 8                                       # YIN gives up where the vibrato is steepest
        dev, base = _cents(got[b, :F], f0[b], sel), _cents(want[b, :F], f0[b], sel)
        print('pitch at %g Hz: device %.3f cents, reference waveform %.3f cents, %d frames' % (hz, dev, base, sel.sum()))
        assert dev <= max(5.0, 2.0 * base)


def test_unvoiced_level():
    """One all-unvoiced second, fixed seed: the frame-averaged |STFT|^2 of the output against exp(2 env_log), both smoothed
    over 9 bins.  Cap: the float64 restatement's figure for the same seed -- the same noise through the same circular filter
    -- plus 0.5 dB."""
    import audio_lib
    import diff_ref
    F = 201
    amp = np.repeat(R.vowel(120.0, 1)[0][None], F, axis=1).astype(np.float32)
    out = audio_lib.hnm_synth_batch(amp, np.zeros((1, F), np.float32), seed=11)
    y = out.y.cpu().numpy()[0]
    env_log = out.env_log.cpu().numpy()[0].astype(np.float64)
    w = R.window(400, 400)
    G = np.exp(env_log) / np.sqrt((w * w).sum())
    ref = diff_ref.istft_frames(diff_ref.synthesis_frames(G * diff_ref.stft(R.noise(11, 0, len(y)), w, HOP), w), w, HOP)
    box = np.ones(9) / 9.0

    def level(x):
        P = (R.stft_mag(x, w, HOP)[R.EDGE:-R.EDGE] ** 2).mean(axis=0)
        d = 10.0 * np.log10(np.convolve(P, box, 'valid') / np.convolve(np.exp(2.0 * env_log).mean(axis=0), box, 'valid'))
        return float(np.sqrt((d ** 2).mean()))

    dev, base = level(y), level(ref)
    print('unvoiced level: device %.3f dB rms, float64 restatement %.3f dB rms' % (dev, base))
    assert dev <= base + 0.5


# ------------------------------------------------------------------------------------------ conversion
def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_convert_hnm_batch(f32_models):
    """conversion.convert_hnm_batch on the tiny random-weight decoder of the conversion tests: the spectra are
    convert_batch(vocode=False)'s bit for bit, the waveform is the composition of the public calls on the same tensors bit for
    bit, the source's contour is the tracker's aligned by the plan, a number scales it, lengths and zeros, out_sr."""
    import _vc
    import audio_lib
    import conversion
    import evaluation
    dec, wd, enc_cfg, dec_cfg, c = f32_models
    wav, lens = _ragged()
    sr, hop = c['sample_rate'], c['hop_length']
    plain = conversion.convert_batch(dec, wav, lens, c, vocode=False)
    r = conversion.convert_hnm_batch(dec, wav, lens, c, seed=5)
    assert r.y_wav_true is None and r.n_frames == plain.n_frames and r.n_samples == plain.n_samples
    for name in ('mel_true', 'mel_pred', 'stft_true', 'stft_pred', 'phn_pred'):
        assert _same(getattr(r, name), getattr(plain, name)), name
    B, Fout, nb = r.stft_pred.shape
    # the source's contour: the tracker on the input, output frame u = input frame n_s + u
    plan = conversion.convert_plan(lens, c)
    f = evaluation.f0_track_batch(wav, lens, sr=sr, hop_length=hop).f0.cpu().numpy()
    want = np.zeros((B, Fout), np.float32)
    for b in range(B):
        n = min(int(plan.n_out[b]), int(plan.n_src[b]) - int(plan.n_s[b]))
        want[b, :n] = f[b, int(plan.n_s[b]):int(plan.n_s[b]) + n]
    assert np.array_equal(r.f0_target.cpu().numpy(), want) and (want > 0).any()
    # the waveform: the public calls on the same tensors
    d_nf = _dev(np.asarray(r.n_frames, np.int32))
    amp = torch.empty_like(r.stft_pred)
    _vc.check(_vc.lib().vc_power_to_amp(_vc.ptr(r.stft_pred), _vc.ptr(d_nf), B, Fout, nb, float(c['P_dB_norm_factor']), 1.0,
                                        _vc.ptr(amp), _vc.current_stream()))
    syn = audio_lib.hnm_synth_batch(amp, r.f0_target, r.n_frames, sr=sr, win_length=c['win_length'], hop_length=hop,
                                    n_fft=c['n_fft'], seed=5)
    assert _same(syn.env_log, r.env_log) and _same(syn.plan.phase, r.plan.phase) and _same(syn.plan.inc, r.plan.inc)
    y = syn.y.clone()
    vplan = audio_lib._get_voc_plan(c['win_length'], hop, c['n_fft'])
    _vc.check(_vc.lib().vc_inv_preemphasis_normalize(vplan.handle, _vc.ptr(y), _vc.ptr(d_nf), B, Fout, y.shape[1],
                                                     float(c['pre_emphasis']), float(15 * c['mean_abs_amp_norm']),
                                                     _vc.current_stream()))
    assert _same(r.y_wav_pred, y)
    yh = r.y_wav_pred.cpu().numpy()
    for b in range(B):
        assert r.n_samples[b] == hop * (r.n_frames[b] - 1) and not yh[b, r.n_samples[b]:].any()
        assert np.isfinite(yh[b]).all() and np.abs(yh[b, :r.n_samples[b]]).max() > 0
    # a number scales the source's contour; a contour is taken as it is; realse != 1 takes vc_power_to_amp
    r2 = conversion.convert_hnm_batch(dec, wav, lens, c, pitch=1.25, seed=5)
    assert torch.equal(r2.f0_target, r.f0_target * 1.25) and _same(r2.stft_pred, r.stft_pred)
    r3 = conversion.convert_hnm_batch(dec, wav, lens, c, pitch=want, seed=5)
    assert _same(r3.y_wav_pred, r.y_wav_pred) and _same(r3.f0_target, r.f0_target)
    r4 = conversion.convert_hnm_batch(dec, wav, lens, c, pitch=want, seed=5, realse=1.2, noise_level=0.0)
    assert r4.plan is not None and np.isfinite(r4.y_wav_pred.cpu().numpy()).all() and not _same(r4.env_log, r.env_log)
    # out_sr
    r5 = conversion.convert_hnm_batch(dec, wav, lens, c, pitch=want, seed=5, out_sr=22050)
    assert r5.n_samples == [int(v) for v in audio_lib.resample_len(np.asarray(r.n_samples), sr, 22050)]
    y5 = r5.y_wav_pred.cpu().numpy()
    assert all(not y5[b, n:].any() and np.abs(y5[b, :n]).max() > 0 for b, n in enumerate(r5.n_samples))
