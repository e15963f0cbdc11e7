"""The general front-end kernels (csrc/vc_frontend.hip) alone on the MI355X, against the float64 reference of
tests/frontend_general_ref.py on the configurations and inputs of tests/frontend_general_cases.py.

Stages are driven one at a time through vc_frontend_stages_f32 with plans of this file's own; every output and the
workspace sit inside larger buffers with a sentinel band on both sides, checked after each call.  Tolerances are those of
tests/test_frontend_gpu.py (dB tolerance times the output's factor; raw stage-2 dB at the unit-factor tolerance); tile sums
of |x| get n * 2^-24 relative, n the number of samples summed.  Raw dB values are compared from 80 dB under the utterance's
maximum upwards: nothing below that can reach an output (top_db), and float32 has no headroom there."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import poison_gpu_state
import frontend_general_cases as fc
import frontend_general_ref as ref

pytestmark = pytest.mark.gpu

BAND = 1024                                 # sentinel floats on each side of a guarded buffer
SENT = np.float32(-98765.4375)              # no kernel here computes this value
NAN = float('nan')


# ------------------------------------------------------------------------------------------ plumbing
class Guarded:
    """n float32 inside a larger device buffer that is filled with the sentinel; .t is the inner view."""

    def __init__(self, n):
        import torch
        self.full = torch.full((n + 2 * BAND,), float(SENT), dtype=torch.float32, device='cuda')
        self.t = self.full[BAND:BAND + n]

    def check(self, what):
        assert bool((self.full[:BAND] == float(SENT)).all()) and bool((self.full[-BAND:] == float(SENT)).all()), \
            'sentinel band overwritten around ' + what

    def numpy(self):
        return self.t.cpu().numpy()


class Plan:
    def __init__(self, kw):
        import _vc
        self.kw = kw
        cfg = _vc.FrontendCfg(int(kw['sr']), int(kw['hop_length']), int(kw['win_length']), ref.n_fft_of(kw), int(kw['n_mels']),
                              int(kw['n_mfcc']), float(kw['pre_emphasis']), float(kw['mean_abs_amp_norm']),
                              float(kw['mfcc_norm_factor']), float(kw['M_dB_norm_factor']), float(kw['P_dB_norm_factor']),
                              int(kw['mfcc_normaleze_first_mfcc']), int(kw['calc_mfcc_derivate']), int(kw['clip_output']))
        self._w = np.ascontiguousarray(ref.window_taps(kw['window'], kw['win_length']), dtype=np.float64)
        self.handle = C.c_void_p()
        _vc.check(_vc.lib().vc_frontend_plan_create(C.byref(cfg), _vc.ptr(self._w), C.byref(self.handle)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import _vc
        import torch
        torch.cuda.synchronize()
        _vc.lib().vc_frontend_plan_destroy(self.handle)


class Call:
    """Buffers of one vc_frontend_stages_f32 call on a ragged batch: guarded outputs and workspace, all sentinel-filled."""

    def __init__(self, plan, lens, max_samples):
        import _vc
        import torch
        kw = plan.kw
        self.plan, self.kw, self.lens, self.B, self.max_samples = plan, kw, list(lens), len(lens), max_samples
        self.NB, self.NM = 1 + ref.n_fft_of(kw) // 2, kw['n_mels']
        self.W = kw['n_mfcc'] * (2 if kw['calc_mfcc_derivate'] else 1)
        self.G = ref.tile_frames(ref.n_fft_of(kw))
        self.o_partial, self.o_stats, self.o_mel, self.total, self.nt, self.mf = ref.ws_layout(kw, self.B, max_samples)
        # the layout restated is the library's
        assert _vc.lib().vc_frontend_workspace_bytes(plan.handle, self.B, max_samples) == self.total
        self.F = [ref.num_frames(L, kw['hop_length']) for L in self.lens]
        self.mfcc, self.mel, self.pow = (Guarded(self.B * self.mf * w) for w in (self.W, self.NM, self.NB))
        self.ws = Guarded(self.total // 4)
        self.d_lens = torch.tensor(self.lens, dtype=torch.int32, device='cuda')

    def run(self, d_wav, stride, mask):
        import _vc
        import torch
        rc = _vc.lib().vc_frontend_stages_f32(self.plan.handle, _vc.ptr(d_wav), _vc.ptr(self.d_lens), self.B, self.max_samples,
                                              stride, 0, _vc.ptr(self.mfcc.t), _vc.ptr(self.mel.t), _vc.ptr(self.pow.t),
                                              _vc.ptr(self.ws.t), self.total, _vc.current_stream(), mask)
        _vc.check(rc)
        torch.cuda.synchronize()
        for g, n in ((self.mfcc, 'd_mfcc'), (self.mel, 'd_mel_db'), (self.pow, 'd_pow_db'), (self.ws, 'the workspace')):
            g.check(n)

    # views of a workspace image (numpy float32 [total / 4])
    def partials(self, ws):
        return ws[self.o_partial // 4:self.o_partial // 4 + self.B * ref.NPART].reshape(self.B, ref.NPART)

    def records(self, ws):
        return ws[self.o_stats // 4:self.o_stats // 4 + self.B * self.nt * ref.STAT].reshape(self.B, self.nt, ref.STAT)

    def mel_raw(self, ws):
        return ws[self.o_mel // 4:self.o_mel // 4 + self.B * self.mf * self.NM].reshape(self.B, self.mf, self.NM)


def _nan_padded_wav(wav, lens, slack):
    """[B, max(lens) + slack] device float32: NaN wherever no utterance has a sample (beyond each length, and the slack)."""
    import torch
    h = np.full((len(lens), max(lens) + slack), NAN, np.float32)
    for b, L in enumerate(lens):
        h[b, :L] = wav[b, :L]
    return torch.from_numpy(h).cuda()


def _up(worst, err):
    """Running maximum that keeps a NaN (Python's max() drops one)."""
    return float(np.maximum(worst, err))


def _measured(what, err, bound):
    print('MEASURED %s: error %.3e bound %.3e ratio %.3f' % (what, err, bound, err / bound if bound else 0.0))
    assert err <= bound, '%s: error %.3e > bound %.3e' % (what, err, bound)


@functools.lru_cache(maxsize=None)
def _stage2_ref(cid, pre):
    kw = dict(fc.kw_of(cid), pre_emphasis=pre)
    wav, lens = fc.inputs(cid)
    return tuple(ref.stage2(wav[b, :L], kw) for b, L in enumerate(lens))


def _is_sent(a):
    return a.view(np.uint32) == SENT.view(np.uint32)


# ------------------------------------------------------------------------------------------ stage 2 alone
@pytest.mark.parametrize('pre', (0.97, 0.0))
@pytest.mark.parametrize('cid', fc.NOT_FAST400)
def test_stage2_alone(cid, pre):
    """stage_mask = 2 on sentinel-filled buffers, the waveform NaN beyond every utterance and in the slack of a row stride
    larger than max_samples: raw power dB rows, raw mel dB rows and every tile record against the reference; rows of frames
    >= F, the partials, the records' unused floats, d_mfcc and d_mel_db untouched; tiles at or beyond F neutral."""
    kw = dict(fc.kw_of(cid), pre_emphasis=pre)
    wav, lens = fc.inputs(cid)
    want = _stage2_ref(cid, pre)
    with Plan(kw) as plan:
        c = Call(plan, lens, max(lens))
        c.run(_nan_padded_wav(wav, lens, 37), max(lens) + 37, 2)
        ws, powd = c.ws.numpy(), c.pow.numpy().reshape(c.B, c.mf, c.NB)
        assert _is_sent(c.mfcc.numpy()).all() and _is_sent(c.mel.numpy()).all()
        touched = np.zeros(ws.shape, bool)
        c.records(touched)[:, :, :5] = True
        meld, rec = c.mel_raw(ws), c.records(ws)
        worst = dict(pow=0.0, mel=0.0, ext_pow=0.0, ext_mel=0.0, sum=0.0)
        for b, L in enumerate(lens):
            F = c.F[b]
            p64, m64, r64 = want[b]
            c.mel_raw(touched)[b, :F] = True
            assert _is_sent(powd[b, F:]).all() and np.isfinite(powd[b, :F]).all() and np.isfinite(meld[b, :F]).all()
            pfl, mfl = ref.floors(p64, m64)
            worst['pow'] = _up(worst['pow'], np.abs(np.maximum(powd[b, :F], pfl) - np.maximum(p64, pfl)).max())
            worst['mel'] = _up(worst['mel'], np.abs(np.maximum(meld[b, :F], mfl) - np.maximum(m64, mfl)).max())
            nt_own = (F + c.G - 1) // c.G
            for t in range(c.nt):
                got = rec[b, t].astype(np.float64)
                if t >= nt_own:
                    assert np.array_equal(rec[b, t, :5], np.array(ref.NEUTRAL, np.float32)), (b, t, rec[b, t])
                    continue
                for i, fl, k in ((0, pfl, 'ext_pow'), (1, pfl, 'ext_pow'), (2, mfl, 'ext_mel'), (3, mfl, 'ext_mel')):
                    worst[k] = _up(worst[k], abs(max(got[i], fl) - max(r64[t, i], fl)))
                if ref.fused_abs(kw):
                    n = min((t + 1) * c.G * kw['hop_length'], L) - t * c.G * kw['hop_length']
                    if r64[t, 4] == 0.0:
                        assert got[4] == 0.0
                    else:
                        worst['sum'] = _up(worst['sum'], abs(got[4] - r64[t, 4]) / (n * 2.0 ** -24 * r64[t, 4]))
        assert _is_sent(ws[~touched]).all(), 'stage 2 wrote outside the valid mel rows and the records'
        tag = '%s pre %.2f stage 2' % (cid, pre)
        _measured(tag + ' raw power dB', worst['pow'], fc.DB_TOL['pow'])
        _measured(tag + ' raw mel dB', worst['mel'], fc.DB_TOL['mel'])
        _measured(tag + ' record power extremes', worst['ext_pow'], fc.DB_TOL['pow'])
        _measured(tag + ' record mel extremes', worst['ext_mel'], fc.DB_TOL['mel'])
        _measured(tag + ' record sum|x| / (n 2^-24 sum)', worst['sum'], 1.0)


# ------------------------------------------------------------------------------------------ stage 1 alone
@pytest.mark.parametrize('cid', fc.ABSSUM_IDS + ('tiny', 'hop160'))
def test_stage1_alone(cid):
    """stage_mask = 1 with mean_abs_amp_norm = 0.003: where hop > n_fft/2 the 16 partials against the reference and nothing
    else written; where stage 2 sums |x| itself, nothing written at all."""
    kw = dict(fc.kw_of(cid), mean_abs_amp_norm=0.003)
    wav, lens = fc.inputs(cid)
    with Plan(kw) as plan:
        c = Call(plan, lens, max(lens))
        c.run(_nan_padded_wav(wav, lens, 5), max(lens) + 5, 1)
        ws = c.ws.numpy()
        assert all(_is_sent(g.numpy()).all() for g in (c.mfcc, c.mel, c.pow))
        touched = np.zeros(ws.shape, bool)
        if cid in fc.ABSSUM_IDS:
            c.partials(touched)[:] = True
            worst = 0.0
            for b, L in enumerate(lens):
                want = ref.abssum_partials(wav[b, :L])
                chunk = (L + ref.NPART - 1) // ref.NPART
                for k in range(ref.NPART):
                    n = max(0, min(L, (k + 1) * chunk) - k * chunk)
                    got = float(c.partials(ws)[b, k])
                    if n == 0 or want[k] == 0.0:
                        assert got == 0.0
                    else:
                        worst = _up(worst, abs(got - want[k]) / (n * 2.0 ** -24 * want[k]))
            _measured('%s stage 1 partials / (n 2^-24 sum)' % cid, worst, 1.0)
        assert _is_sent(ws[~touched]).all()


# ------------------------------------------------------------------------------------------ stage 3 alone
def _stage3_call(plan, cid, data, records_of, partials_of):
    """Writes raw dB rows, records and partials of four utterances (NaN wherever stage 3 must not read: rows of frames >= F,
    the records' unused floats, the waveform), runs stage_mask = 4 and returns (call, [reference outputs])."""
    import torch
    kw = plan.kw
    lens = fc.exact_lens(cid)
    c = Call(plan, lens, max(lens))
    ws = np.full(c.total // 4, NAN, np.float32)
    powd = np.full((c.B, c.mf, c.NB), NAN, np.float32)
    want = []
    for b, L in enumerate(lens):
        p, m = data[b]
        F = c.F[b]
        rec = records_of(b, p, m, c)
        par = partials_of(b, L)
        powd[b, :F], c.mel_raw(ws)[b, :F] = p, m
        c.records(ws)[b, :, :5] = rec
        c.partials(ws)[b] = par
        want.append(ref.stage3(p, m, rec, par, L, kw))
    c.pow.t.copy_(torch.from_numpy(powd.ravel()))
    c.ws.t.copy_(torch.from_numpy(ws))
    d_wav = torch.full((c.B, max(lens)), NAN, dtype=torch.float32, device='cuda')
    c.run(d_wav, max(lens), 4)
    return c, want


def _stage3_outputs(c):
    return (c.mfcc.numpy().reshape(c.B, c.mf, c.W), c.mel.numpy().reshape(c.B, c.mf, c.NM),
            c.pow.numpy().reshape(c.B, c.mf, c.NB))


@pytest.mark.parametrize('name', fc.EXACT_SETS)
@pytest.mark.parametrize('cid', fc.EXACT_IDS)
def test_stage3_alone_exact_cases(cid, name):
    """stage_mask = 4 on hand-written raw dB (1/8 dB grid, factors 1/128, mean_abs_amp_norm 1): power and mel outputs bit
    for bit, MFCC and delta to tolerance, rows beyond F exactly zero.  'nan_padding' puts NaN into the records of tiles at
    or beyond F (the other sets: the neutral record)."""
    kw = fc.exact_kw(cid)

    def records_of(b, p, m, c):
        nt_own = (c.F[b] + c.G - 1) // c.G
        rec = ref.tile_records(p, m, np.zeros(nt_own), c.G, c.nt)
        if name == 'nan_padding':
            rec[nt_own:] = NAN
        return rec

    with Plan(kw) as plan:
        c, want = _stage3_call(plan, cid, fc.exact_data(cid, name), records_of, lambda b, L: np.full(ref.NPART, NAN))
        mfcc, mel, powd = _stage3_outputs(c)
        worst = 0.0
        for b in range(c.B):
            F = c.F[b]
            wc, wm, wp = want[b]
            assert np.array_equal(mel[b, :F], wm.astype(np.float32)), (cid, name, b, 'mel')
            assert np.array_equal(powd[b, :F], wp.astype(np.float32)), (cid, name, b, 'pow')
            assert not mfcc[b, F:].any() and not mel[b, F:].any() and not powd[b, F:].any()
            assert np.isfinite(mfcc[b]).all()
            worst = _up(worst, np.abs(mfcc[b, :F] - wc).max())
            if name == 'below_amin':
                assert not mel[b].any() and not powd[b].any()
        _measured('%s %s stage 3 MFCC / delta' % (cid, name), worst, fc.tol('mfcc', kw))


@pytest.mark.parametrize('cid', fc.EXACT_IDS)
def test_stage3_alone_amplitude_offset(cid):
    """mean_abs_amp_norm = 0.003 with sum|x| spread unevenly over the tile records -- over the 16 partials where stage 1
    runs, the records' sums then holding 1e30 that must not be read: the offsets 20 log10 c and 40 log10 c to tolerance."""
    kw = fc.exact_kw(cid, norm=0.003)
    fused = ref.fused_abs(kw)

    def records_of(b, p, m, c):
        nt_own = (c.F[b] + c.G - 1) // c.G
        share = 0.5 ** np.arange(nt_own)
        asum = 0.05 * (b + 1) * fc.exact_lens(cid)[b] * share / share.sum()
        return ref.tile_records(p, m, asum if fused else np.full(nt_own, 1e30), c.G, c.nt)

    def partials_of(b, L):
        if fused:
            return np.full(ref.NPART, NAN)
        share = np.arange(1.0, ref.NPART + 1) ** 2
        return 0.05 * (b + 1) * L * share / share.sum()

    with Plan(kw) as plan:
        c, want = _stage3_call(plan, cid, fc.exact_data(cid, 'range30'), records_of, partials_of)
        got = _stage3_outputs(c)
        worst = dict(mfcc=0.0, mel=0.0, pow=0.0)
        for b in range(c.B):
            F = c.F[b]
            for n, g, w in zip(('mfcc', 'mel', 'pow'), got, want[b]):
                assert not g[b, F:].any()
                worst[n] = _up(worst[n], np.abs(g[b, :F] - w).max())
        for n in worst:
            _measured('%s stage 3 with offset, %s' % (cid, n), worst[n], fc.tol(n, kw))


# ------------------------------------------------------------------------------------------ all stages, public API
def _public_checks(cid, name, kw, poison):
    import torch
    import _vc
    import audio_lib
    wav, lens = fc.inputs(cid)
    s2 = _stage2_ref(cid, kw['pre_emphasis'])
    d_wav = torch.from_numpy(wav.copy()).cuda()
    out = audio_lib.calc_MFCC_input_batch(d_wav, list(lens), **kw)
    Fmax = 1 + wav.shape[1] // kw['hop_length']
    worst = dict(mfcc=0.0, mel=0.0, pow=0.0)
    for b, L in enumerate(lens):
        F = ref.num_frames(L, kw['hop_length'])
        want = ref.stage3(s2[b][0], s2[b][1], s2[b][2], ref.abssum_partials(wav[b, :L]), L, kw)
        alone = audio_lib.calc_MFCC_input_batch(d_wav[b:b + 1, :L].contiguous(), None, **kw)
        for n, t, a, w in zip(('mfcc', 'mel', 'pow'), out, alone, want):
            assert t.shape[:2] == (len(lens), Fmax) and t.dtype == torch.float32
            assert torch.equal(t[b, :F], a[0]), (cid, name, b, n, 'row b of the batch differs from utterance b alone')
            assert float(t[b, F:].abs().max()) == 0.0 if F < Fmax else True
            worst[n] = _up(worst[n], np.abs(t[b, :F].cpu().numpy() - w).max())
    for n in worst:
        _measured('%s-%s all stages, %s' % (cid, name, n), worst[n], fc.tol(n, kw))
    if poison:
        poison_gpu_state()
        again = audio_lib.calc_MFCC_input_batch(d_wav, list(lens), **kw)
        assert all(torch.equal(a, o) for a, o in zip(again, out)), (cid, name, 'a second run differs')
    if fc.CASES[cid][1] != 'fast400':
        with pytest.raises(_vc.VCError):
            audio_lib.calc_MFCC_input_batch(d_wav, list(lens), out_frames=Fmax - 1, **kw)


@pytest.mark.parametrize('cid,name', fc.ALL_VARIANTS, ids=['%s-%s' % v for v in fc.ALL_VARIANTS])
def test_all_stages_public_api(cid, name):
    """audio_lib.calc_MFCC_input_batch on the ragged batch: every utterance against the float64 reference, row b equal to
    utterance b run alone bit for bit, padding rows exactly zero, out_frames < Fmax refused off the shipped path, and (first
    flag set of every id) a second run after poison_gpu_state() bit-identical.  The shipped path with the 8 kHz mel table
    runs in both of its forms."""
    import _vc
    kw = fc.variant_kw(cid, name)
    first = name == fc.variants(cid)[0][0]
    if fc.CASES[cid][1] == 'fast400':
        for fused in (1, 0):
            with _vc.options(fe_fused=fused):
                _public_checks(cid, '%s fe_fused=%d' % (name, fused), kw, first)
    else:
        _public_checks(cid, name, kw, first)


@pytest.mark.parametrize('cid', fc.OVER_64K)
def test_above_64k_of_lds_is_served(cid):
    """The launches that ask for more than 64 KB of dynamic LDS (finalize at 128 mels with 80 or 128 cepstra, the 400-point
    kernel at hop 560, the generic kernel at n_fft 2048) return correct features: every one has the opt-in."""
    lds = ref.lds_bytes(fc.kw_of(cid))
    assert {k: lds[k] for k in fc.CASES[cid][2]} == fc.LDS_FACTS[cid] and all(v > 64 * 1024 for v in fc.LDS_FACTS[cid].values())
    _public_checks(cid, 'listed (%s: %s B)' % (', '.join(fc.LDS_FACTS[cid]), ', '.join(str(v) for v in fc.LDS_FACTS[cid].values())),
                   fc.kw_of(cid), False)
