"""The scoring launches alone, through the C ABI with raw pointers: vc_mel_cepstra, vc_dtw_f32, vc_dtw_backtrack and
vc_frame_mcd_f32 of csrc/vc_dtw.hip; vc_f0_yin_f32, vc_f0_candidates_f32 and vc_f0_metrics_f32 of csrc/vc_f0.hip;
vc_frame_energy_f32, vc_activity_mask, vc_mask_compact, vc_compact_rows_f32, vc_path_map, vc_speech_gain_f32 and
vc_scale_rows_f32 of csrc/vc_activity.hip -- against tests/mcd_ref.py, tests/f0_ref.py and tests/activity_ref.py on the
cases of tests/score_kernels_cases.py (tests/test_score_kernels_cpu.py proves those usable and pins the bounds).

The memory contract of every test: it starts with poison_gpu_state(); every output and every workspace lies between two
bands of sentinels that are checked after each call; a workspace is exactly as long as the size query says; outputs
start as NaN (sentinel integers); inputs hold NaN (0x7fffffff, active mask bytes) wherever the header says the kernel
does not read -- behind lens[b], in the slack max_len .. ld, in the rows past a pair's lengths; every launch runs twice
and the raw bits agree; row b of the ragged batch in those dirty buffers equals, bit for bit, utterance b run alone in
tight, clean ones.  Exact cases are compared bit for bit; a real-valued one prints a line starting with MEASURED with
its error, bound and ratio (profiles/score_kernels/README.md records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import activity_ref as ar
import f0_ref as fr
import mcd_ref as mr
import score_kernels_cases as Cs
from conftest import poison_gpu_state

pytestmark = pytest.mark.gpu

VC_ERR_INVALID, VC_ERR_WORKSPACE, VC_ERR_UNSUPPORTED = 1, 3, 4
VC_F32, VC_BF16 = 0, 1
CAN32, CAN8 = 0x7FA5A5A5, 0xA5          # NaN with a payload no arithmetic produces; as an integer, a number no case holds
BAND = 256                              # sentinel bytes on either side (keeps a workspace's 16-byte alignment)
IFILL = 0x7FFFFFFF
EPS = Cs.EPS


def _lib():
    import _vc
    return _vc.lib()


def _st():
    import _vc
    return _vc.current_stream()


def _ok(rc):
    import _vc
    _vc.check(rc)
    torch.cuda.synchronize()


def _refused(rc, code, text=''):
    msg = _lib().vc_last_error().decode()
    assert rc == code and text in msg, (rc, code, msg)


class Buf:
    """n elements of float32 / int32 ('f', 'i': four bytes) or bytes ('b') between two bands of sentinels."""

    def __init__(self, n, kind='f'):
        self.n, self.kind = int(n), kind
        self.idt, self.can, self.pad = (torch.uint8, CAN8, BAND) if kind == 'b' else (torch.int32, CAN32, BAND // 4)
        self.raw = torch.full((self.n + 2 * self.pad,), self.can, dtype=self.idt, device='cuda')

    def ptr(self, off=0):
        return C.c_void_p(self.raw.data_ptr() + self.pad * self.raw.element_size() + off)

    def bands_ok(self):
        torch.cuda.synchronize()
        return bool((self.raw[:self.pad] == self.can).all()) and bool((self.raw[self.pad + self.n:] == self.can).all())

    def bits(self, shape=None, written=True):
        """The body's bits on the host (int32 or uint8); the bands must be intact and, by default, no sentinel left inside."""
        assert self.bands_ok(), 'wrote outside the buffer'
        body = self.raw[self.pad:self.pad + self.n].cpu().numpy().copy()
        if written and self.kind != 'b':
            assert not (body == self.can).any(), '%d elements were never written' % int((body == self.can).sum())
        return body if shape is None else body.reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == self.can).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def i32(v):
    return dev(np.asarray(v, dtype=np.int32))


def f32(bits):
    return bits.view(np.float32)


def padded(rows, width, fill, dtype=np.float32, tail=()):
    """[len(rows), width] + tail with row b's data first and `fill` everywhere else."""
    out = np.full((len(rows), width) + tuple(tail), fill, dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


@pytest.fixture(autouse=True)
def _own_line():
    print()                                                              # (-s: the MEASURED lines start their own line)
    yield


def twice(run, what):
    """run() -> dict of host bit arrays: two launches into fresh sentinels, identical bits; the first one's."""
    a, b = run(), run()
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), '%s: two launches differ in %s' % (what, k)
    return a


def measured(what, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
    print('MEASURED %s err=%.3e bound=%.3e err/bound=%.3f' % (what, err, bound, ratio))
    return ratio


# ================================================================================================ DTW
def run_dtw(pairs, n_coef, scale=1.0, band=-1, want_path=1, dirty=True, lens=None):
    lib, st = _lib(), _st()
    B = len(pairs)
    Fa, Fb = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    max_a, max_b = (max(Fa) + Cs.DTW_PAD_A, max(Fb) + Cs.DTW_PAD_B) if dirty else (max(Fa), max(Fb))
    fill = np.nan if dirty else 0.0
    ca = dev(padded([a for a, _ in pairs], max_a, fill, tail=(n_coef,)))
    cb = dev(padded([b for _, b in pairs], max_b, fill, tail=(n_coef,)))
    la, lb = (i32(Fa), i32(Fb)) if lens is None else (i32(lens[0]), i32(lens[1]))
    nbytes = lib.vc_dtw_workspace_size(B, max_a, max_b, want_path)
    assert nbytes > 0 and nbytes % 16 == 0
    ws = Buf(nbytes, 'b')                                                # exactly what the size query says
    total, plen, mcd = Buf(B), Buf(B, 'i'), Buf(B)
    _ok(lib.vc_dtw_f32(ptr(ca), ptr(cb), ptr(la), ptr(lb), B, max_a, max_b, n_coef, scale, band, want_path, total.ptr(), plen.ptr(),
                       mcd.ptr(), ws.ptr(), nbytes, st))
    assert ws.bands_ok(), 'wrote outside the workspace'
    out = dict(total=total.bits(), path_len=plen.bits(), mcd=mcd.bits())
    if want_path:
        path = Buf(B * (max_a + max_b - 1) * 2, 'i')
        _ok(lib.vc_dtw_backtrack(ws.ptr(), nbytes, ptr(la), ptr(lb), total.ptr(), plen.ptr(), B, max_a, max_b, path.ptr(), st))
        assert ws.bands_ok() and total.bands_ok()
        out['path'] = path.bits((B, max_a + max_b - 1, 2))
    return out


def check_exact_pair(res, b, ref, what):
    total, n, path = ref
    got_t, got_n = float(f32(res['total'])[b]), int(res['path_len'][b])
    assert got_t == float(total) and got_n == n, (what, got_t, float(total), got_n, n)
    assert f32(res['mcd'])[b] == np.float32(np.float32(total) / np.float32(n)), what
    p = res['path'][b]
    assert np.array_equal(p[:n], path), (what, 'path')
    assert (p[n:] == -1).all(), (what, 'fill behind the path')


def same_pair(batch, b, alone, what, keys=('total', 'path_len', 'mcd')):
    for k in keys:
        assert batch[k][b] == alone[k][0], (what, k)
    if 'path' in batch and 'path' in alone:
        n = int(alone['path_len'][0])
        assert np.array_equal(batch['path'][b][:n], alone['path'][0][:n]), (what, 'path')


@pytest.mark.parametrize('n_coef', [n for n, _ in Cs.DTW_EXACT])
def test_dtw_exact_integer_cases_in_dirty_buffers(n_coef):
    """Totals, lengths and whole paths equal the reference; score mode is bit-identical to path mode; every pair of the
    ragged batch (max_a > Fa, max_b > Fb, NaN rows behind every utterance) equals the pair alone in tight buffers."""
    poison_gpu_state()
    pairs = Cs.dtw_exact_pairs(n_coef)
    res = twice(lambda: run_dtw(pairs, n_coef), 'vc_dtw_f32 path mode')
    score = twice(lambda: run_dtw(pairs, n_coef, want_path=0), 'vc_dtw_f32 score mode')
    for b, (a, c) in enumerate(pairs):
        what = 'n_coef %d, %d x %d' % (n_coef, len(a), len(c))
        check_exact_pair(res, b, Cs.dtw_exact_reference(n_coef, b), what)
        for k in ('total', 'path_len', 'mcd'):
            assert score[k][b] == res[k][b], (what, k, 'score mode against path mode')
        alone = run_dtw([pairs[b]], n_coef, dirty=False)
        same_pair(res, b, alone, what)
        assert (alone['path'][0][int(alone['path_len'][0]):] == -1).all()


def test_dtw_lengths_outside_their_range_are_clamped():
    """include/vc_hip.h: d_len_a / d_len_b are clamped to [1, max]."""
    poison_gpu_state()
    rng = np.random.RandomState(5)
    full = [(Cs.int_cepstra(rng, 9, 8), Cs.int_cepstra(rng, 21, 8)) for _ in range(4)]
    lens = ([0, -7, 9 + 100, 4], [21 + 1, 5, 0x7FFFFFFF, -1])
    res = twice(lambda: run_dtw(full, 8, dirty=False, lens=lens), 'clamped lengths')
    for b, (a, c) in enumerate(full):
        Fa, Fb = min(max(lens[0][b], 1), 9), min(max(lens[1][b], 1), 21)
        check_exact_pair(res, b, mr.dtw(a[:Fa], c[:Fb], 1.0), 'lens %d, %d' % (lens[0][b], lens[1][b]))


@pytest.mark.parametrize('n_coef,shape', Cs.DTW_BAND)
def test_dtw_band_wide_enough_one_too_narrow_and_unreachable(n_coef, shape):
    """A band that just holds the free optimum changes nothing; one narrower equals the banded reference; band = 0 with
    Fa != Fb cannot reach the end cell: a total that is not finite and a path of all -1."""
    poison_gpu_state()
    Fa, Fb = shape
    a, b, free, need = Cs.dtw_band_pair(n_coef, Fa, Fb)
    for band in (need, need - 1, 0):
        ref = Cs.dtw_band_reference(n_coef, Fa, Fb, band)
        res = twice(lambda: run_dtw([(a, b)], n_coef, band=band), 'band %d' % band)
        score = run_dtw([(a, b)], n_coef, band=band, want_path=0)
        assert score['total'][0] == res['total'][0], band
        if np.isfinite(ref[0]):
            check_exact_pair(res, 0, ref, 'band %d' % band)
            assert score['path_len'][0] == res['path_len'][0] and score['mcd'][0] == res['mcd'][0]
            if band == need:
                assert float(f32(res['total'])[0]) == float(free[0]) and np.array_equal(res['path'][0][:free[1]], free[2])
        else:
            assert band == 0 and Fa != Fb
            assert not np.isfinite(f32(res['total'])[0]) and f32(res['total'])[0] > 0
            assert (res['path'][0] == -1).all()
    if Fa != Fb:
        assert not np.isfinite(Cs.dtw_band_reference(n_coef, Fa, Fb, 0)[0])


@pytest.mark.parametrize('n_coef,shape', Cs.DTW_REAL)
def test_dtw_real_valued_cases_within_the_derived_bound(n_coef, shape):
    """_check_real of tests/test_mcd_gpu.py on one pair: (a) a valid path, (b) its float64 cost within 2 (Fa + Fb + n_coef
    + 2) eps of the float64 optimum, (c) the total within half that of its own path's cost, (d) the total's error at most
    3 x the float32 restatement's (or an ulp)."""
    poison_gpu_state()
    Fa, Fb = shape
    a, b, t64, t32 = Cs.dtw_real_pair(n_coef, Fa, Fb)
    res = twice(lambda: run_dtw([(a, b)], n_coef, scale=Cs.REAL_SCALE), 'real-valued')
    total, n = float(f32(res['total'])[0]), int(res['path_len'][0])
    path = res['path'][0][:n]
    assert (res['path'][0][n:] == -1).all()
    mr.check_path(path, Fa, Fb, None)
    bound = Cs.dtw_real_bound(Fa, Fb, n_coef)
    cost = mr.path_cost(a, b, path, Cs.REAL_SCALE)
    gap, own, err, yard = (cost - t64) / t64, abs(total - cost) / cost, abs(total - t64) / t64, abs(t32 - t64) / t64
    ulp = float(np.spacing(np.float32(total))) / total
    measured('vc_dtw_f32 %dx%d nc%d path gap' % (Fa, Fb, n_coef), gap, bound)
    measured('vc_dtw_f32 %dx%d nc%d total vs own path' % (Fa, Fb, n_coef), own, bound / 2)
    measured('vc_dtw_f32 %dx%d nc%d total vs 3x restatement' % (Fa, Fb, n_coef), err, 3.0 * (yard if yard > 0 else ulp))
    assert gap <= bound and own <= bound / 2 and err <= 3.0 * (yard if yard > 0 else ulp), (gap, own, err, yard, ulp, bound)
    assert f32(res['mcd'])[0] == np.float32(np.float32(total) / np.float32(n))
    score = run_dtw([(a, b)], n_coef, scale=Cs.REAL_SCALE, want_path=0)
    alone = run_dtw([(a, b)], n_coef, scale=Cs.REAL_SCALE, dirty=False)
    for k in ('total', 'path_len', 'mcd'):
        assert score[k][0] == res[k][0] and alone[k][0] == res[k][0], k
    assert np.array_equal(alone['path'][0][:n], path)


def test_dtw_refuses_what_the_header_says_it_refuses():
    poison_gpu_state()
    lib, st = _lib(), _st()
    B, max_a, max_b = 2, 40, 50
    ca, cb = dev(np.zeros((B, max_a, 33), np.float32)), dev(np.zeros((B, max_b, 33), np.float32))
    la, lb = i32([40, 3]), i32([50, 7])
    total, plen, mcd = Buf(B), Buf(B, 'i'), Buf(B)
    for want in (0, 1):
        nbytes = lib.vc_dtw_workspace_size(B, max_a, max_b, want)
        ws = Buf(nbytes + 16, 'b')

        def call(n_coef=24, off=0, size=nbytes):
            return lib.vc_dtw_f32(ptr(ca), ptr(cb), ptr(la), ptr(lb), B, max_a, max_b, n_coef, 1.0, -1, want, total.ptr(), plen.ptr(),
                                  mcd.ptr(), ws.ptr(off), size, st)

        _refused(call(n_coef=33), VC_ERR_UNSUPPORTED, 'n_coef 33')
        _refused(call(size=nbytes - 1), VC_ERR_WORKSPACE, 'workspace')
        for off in (4, 8, 1):
            _refused(call(off=off), VC_ERR_INVALID, 'unaligned')
        assert ws.untouched() and total.untouched() and plen.untouched() and mcd.untouched()
    nbytes = lib.vc_dtw_workspace_size(B, max_a, max_b, 1)
    ws, path = Buf(nbytes, 'b'), Buf(B * (max_a + max_b - 1) * 2, 'i')
    _refused(lib.vc_dtw_backtrack(ws.ptr(), nbytes - 1, ptr(la), ptr(lb), total.ptr(), plen.ptr(), B, max_a, max_b, path.ptr(), st),
             VC_ERR_WORKSPACE, 'workspace')
    assert path.untouched()
    assert lib.vc_dtw_workspace_size(B, 0, max_b, 0) == 0 and lib.vc_dtw_workspace_size(B, max_a, 16385, 1) == 0


# ================================================================================================ frame MCD, cepstra
def run_frame_mcd(pairs, n_coef, dirty=True):
    B = len(pairs)
    Fa, Fb = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    max_a, max_b = (max(Fa) + Cs.FRAME_PAD_A, max(Fb) + Cs.FRAME_PAD_B) if dirty else (max(Fa), max(Fb))
    fill = np.nan if dirty else 0.0
    ca = dev(padded([a for a, _ in pairs], max_a, fill, tail=(n_coef,)))
    cb = dev(padded([b for _, b in pairs], max_b, fill, tail=(n_coef,)))
    out = Buf(B)
    la, lb = i32(Fa), i32(Fb)                                            # (named: a temporary's memory is free for the next one)
    _ok(_lib().vc_frame_mcd_f32(ptr(ca), ptr(cb), ptr(la), ptr(lb), B, max_a, max_b, n_coef, Cs.REAL_SCALE, out.ptr(), _st()))
    return dict(mcd=out.bits())


@pytest.mark.parametrize('n_coef', Cs.FRAME_MCD_COEF)
def test_frame_mcd_against_float64(n_coef):
    poison_gpu_state()
    rng = np.random.RandomState(n_coef)
    pairs = [((0.05 * rng.standard_normal((Fa, n_coef))).astype(np.float32), (0.05 * rng.standard_normal((Fb, n_coef))).astype(np.float32))
             for Fa, Fb in Cs.FRAME_MCD_PAIRS]
    assert pairs[0][0].shape[0] != pairs[-1][1].shape[0]
    res = twice(lambda: run_frame_mcd(pairs, n_coef), 'vc_frame_mcd_f32')
    for b, (a, c) in enumerate(pairs):
        n = min(len(a), len(c))
        want = mr.frame_mcd(a, c, Cs.REAL_SCALE)
        err = abs(float(f32(res['mcd'])[b]) - want) / want
        assert measured('vc_frame_mcd_f32 nc%d n%d' % (n_coef, n), err, Cs.frame_mcd_bound(n, n_coef)) <= 1.0
        assert run_frame_mcd([pairs[b]], n_coef, dirty=False)['mcd'][0] == res['mcd'][b], b


def run_cepstra(mel, tab, dtype):
    rows, n_mels = mel.shape
    n_coef = tab.shape[0]
    x = dev(mel.astype(np.float32))
    if dtype == VC_BF16:
        x = x.bfloat16()
    t = dev(tab.astype(np.float32))
    out = Buf(rows * n_coef)
    _ok(_lib().vc_mel_cepstra(ptr(x), dtype, rows, n_mels, ptr(t), n_coef, out.ptr(), _st()))
    return dict(cep=out.bits((rows, n_coef)))


def _bf16_grid(a):
    return torch.from_numpy(a.astype(np.float32)).bfloat16().float().numpy()


@pytest.mark.parametrize('n_mels,n_coef', Cs.CEPSTRA_SHAPES)
def test_mel_cepstra_against_the_float64_product(n_mels, n_coef):
    """Rows 1, 255, 257 in both input types; 512 x 32 takes exactly 64 KB of LDS."""
    poison_gpu_state()
    rng = np.random.RandomState(n_mels)
    tab = mr.dct_table(n_mels, n_coef, 0 if n_coef == n_mels else 1).astype(np.float32)
    for rows in Cs.CEPSTRA_ROWS:
        for dtype in (VC_F32, VC_BF16):
            mel = rng.uniform(0.0, 1.0, (rows, n_mels)).astype(np.float32)
            mel = _bf16_grid(mel) if dtype == VC_BF16 else mel
            got = f32(twice(lambda: run_cepstra(mel, tab, dtype), 'vc_mel_cepstra')['cep']).astype(np.float64)
            want, bound = mr.cepstra(mel, table=tab), Cs.cepstra_bound(tab, mel)
            err = np.abs(got - want)
            k = np.unravel_index(np.argmax(err / bound), err.shape)
            assert measured('vc_mel_cepstra %dx%d->%d %s' % (rows, n_mels, n_coef, 'bf16' if dtype else 'f32'), err[k], bound[k]) <= 1.0


def test_mel_cepstra_second_trip_of_the_grid_stride_loop():
    poison_gpu_state()
    rows, n_mels, n_coef = Cs.CEPSTRA_LONG
    rng = np.random.RandomState(1)
    tab = mr.dct_table(n_mels, n_coef, 1).astype(np.float32)
    mel = rng.uniform(0.0, 1.0, (rows, n_mels)).astype(np.float32)
    got = f32(twice(lambda: run_cepstra(mel, tab, VC_F32), 'vc_mel_cepstra')['cep']).astype(np.float64)
    ratio = np.abs(got - mr.cepstra(mel, table=tab)) / Cs.cepstra_bound(tab, mel)
    assert rows * n_coef > 4096 * 256
    assert measured('vc_mel_cepstra %dx%d->%d second trip' % (rows, n_mels, n_coef), float(ratio.max()), 1.0) <= 1.0
    lib = _lib()
    out = Buf(8)
    z = dev(np.zeros((8, 600), np.float32))
    _refused(lib.vc_mel_cepstra(ptr(z), VC_F32, 1, 8, ptr(z), 9, out.ptr(), _st()), VC_ERR_INVALID, 'bad shape')
    _refused(lib.vc_mel_cepstra(ptr(z), VC_F32, 1, 513, ptr(z), 8, out.ptr(), _st()), VC_ERR_INVALID, 'bad shape')
    _refused(lib.vc_mel_cepstra(ptr(z), VC_F32, 1, 64, ptr(z), 33, out.ptr(), _st()), VC_ERR_INVALID, 'bad shape')
    assert out.untouched()


# ================================================================================================ YIN and candidates
def _wave_batch(rows, dirty, null_lens=False):
    lens = [len(r) for r in rows]
    max_len = max(max(lens), 1)
    ld = max_len + 5 if dirty else max_len
    wav = dev(padded(rows, ld, np.nan if dirty else 0.0))
    return wav, (None if null_lens else i32(lens)), lens, max_len, ld


def run_yin(name, rows, dirty=True, null_lens=False):
    W, hop, tau_min, tau_max = Cs.YIN_CONFIGS[name]
    wav, d_lens, lens, max_len, ld = _wave_batch(rows, dirty, null_lens)
    B = len(rows)
    max_frames = 1 + max_len // hop + ((Cs.yin_tile(W, tau_max, hop) + 3) if dirty else 0)
    f0, ap = Buf(B * max_frames), Buf(B * max_frames)
    _ok(_lib().vc_f0_yin_f32(ptr(wav), ptr(d_lens), B, max_len, ld, Cs.SR, hop, W, tau_min, tau_max, Cs.THRESHOLD, f0.ptr(), ap.ptr(),
                             max_frames, _st()))
    return dict(f0=f0.bits((B, max_frames)), ap=ap.bits((B, max_frames)))


def run_cand(name, rows, n_cand, ceiling=1.0, dirty=True, null_lens=False, cfg=None):
    W, hop, tau_min, tau_max = cfg or Cs.YIN_CONFIGS[name]
    wav, d_lens, lens, max_len, ld = _wave_batch(rows, dirty, null_lens)
    B = len(rows)
    max_frames = 1 + max_len // hop + ((Cs.yin_tile(W, tau_max, hop, True) + 3) if dirty else 0)
    f0, pitch, cost = Buf(B * max_frames * n_cand), Buf(B * max_frames * n_cand), Buf(B * max_frames * n_cand)
    n, ap = Buf(B * max_frames, 'i'), Buf(B * max_frames)
    _ok(_lib().vc_f0_candidates_f32(ptr(wav), ptr(d_lens), B, max_len, ld, Cs.SR, hop, W, tau_min, tau_max, ceiling, n_cand, f0.ptr(),
                                    pitch.ptr(), cost.ptr(), n.ptr(), ap.ptr(), max_frames, _st()))
    s3 = (B, max_frames, n_cand)
    return dict(f0=f0.bits(s3), pitch=pitch.bits(s3), cost=cost.bits(s3), n=n.bits((B, max_frames)), ap=ap.bits((B, max_frames)))


ONE = np.float32(1.0).view(np.int32)


def check_yin_rows(name, res, rows):
    """The rule of test_a_ragged_batch_against_the_float64_definition, with delta from this configuration's W + tau_max
    (f0_ref.yin computes the floors from the W and tau_max it is given)."""
    W, hop, tau_min, tau_max = Cs.YIN_CONFIGS[name]
    worst_c = worst_a = 0.0
    bound_c = bound_a = 0.0
    for b, ((f64, a64, det), (f32r, a32r)) in enumerate(Cs.yin_reference(name)):
        F = 1 + len(rows[b]) // hop
        f0, ap = f32(res['f0'])[b], f32(res['ap'])[b]
        assert (res['f0'][b, F:] == 0).all() and (res['ap'][b, F:] == ONE).all(), (name, b, 'frames past the utterance')
        keep = ~det['marginal']
        assert det['marginal'].sum() <= (0.01 * F if F >= 100 else 0)
        assert np.array_equal(f0[:F][keep] > 0, f64[keep] > 0), (name, b, np.nonzero((f0[:F] > 0) != (f64 > 0))[0][:10])
        both = keep & (f64 > 0) & (f32r > 0) & (f0[:F] > 0)
        e_a, y_a = np.abs(ap[:F].astype(np.float64) - a64), np.abs(a32r.astype(np.float64) - a64)
        if both.any():
            e_c, y_c = np.abs(fr.cents(f0[:F][both], f64[both])).max(), np.abs(fr.cents(f32r[both], f64[both])).max()
            lim = 3.0 * (y_c if y_c > 0 else det['floor_cents'][both].max())
            assert e_c <= lim, (name, b, e_c, y_c)
            if lim > 0 and e_c / lim >= worst_c:
                worst_c, bound_c = e_c / lim, lim
        if keep.any():
            ya = y_a[keep].max()
            lim = 3.0 * (ya if ya > 0 else det['floor_ap'][keep].max())
            assert e_a[keep].max() <= lim, (name, b, e_a[keep].max(), ya)
            if lim > 0 and e_a[keep].max() / lim >= worst_a:
                worst_a, bound_a = e_a[keep].max() / lim, lim
    measured('vc_f0_yin_f32 %s f0 cents' % name, worst_c * bound_c, bound_c)
    measured('vc_f0_yin_f32 %s aperiodicity' % name, worst_a * bound_a, bound_a)


def check_cand_rows(name, res, rows, n_cand):
    """On the frames that are not marginal (f0_track_ref.marginal_frames, with this configuration's W + tau_max): the
    count and the lags of the float64 selection, in ascending lag; cost within 3 x the float32 restatement's error or the
    floor delta * d'; pitch = log2(f0) to an ulp; the empty slots 0, 0, 1; n = 0 and aperiodicity 1 past the utterance."""
    W, hop, tau_min, tau_max = Cs.YIN_CONFIGS[name]
    delta = (W + tau_max) * EPS
    worst = wb = 0.0
    for b, (c64, c32) in enumerate(Cs.cand_reference(name, n_cand)):
        F = 1 + len(rows[b]) // hop
        f0, pitch, cost, n = f32(res['f0'])[b], f32(res['pitch'])[b], f32(res['cost'])[b], res['n'][b]
        assert (n[F:] == 0).all() and (res['ap'][b, F:] == ONE).all(), (name, b)
        assert (res['f0'][b, F:] == 0).all() and (res['pitch'][b, F:] == 0).all() and (res['cost'][b, F:] == ONE).all(), (name, b)
        assert ((n[:F] >= 0) & (n[:F] <= n_cand)).all()
        for f in range(F):
            k = int(n[f])
            assert (f0[f, k:] == 0).all() and (pitch[f, k:] == 0).all() and (cost[f, k:] == 1).all(), (name, b, f)
            assert (f0[f, :k] > 0).all() and (np.diff(f0[f, :k]) < 0).all(), (name, b, f, 'ascending lag')
            want = np.log2(f0[f, :k].astype(np.float64))
            assert (np.abs(pitch[f, :k] - want) <= Cs.LOG2_ULPS * np.spacing(np.abs(want).astype(np.float32))).all(), (name, b, f)
            if c64['marginal'][f]:
                continue
            assert k == c64['n'][f], (name, b, f, k, c64['n'][f])
            lag = Cs.SR / f0[f, :k].astype(np.float64)
            assert (np.abs(lag - c64['lag'][f, :k]) <= 0.5 + 4 * EPS * lag).all(), (name, b, f, lag, c64['lag'][f, :k])
            e = np.abs(cost[f, :k].astype(np.float64) - c64['cost'][f, :k])
            y = np.abs(c32['cost'][f, :k].astype(np.float64) - c64['cost'][f, :k]) if c32['n'][f] == k else np.zeros(k)
            lim = 3.0 * np.where(y > 0, y, delta * c64['cost'][f, :k])
            assert (e <= lim).all(), (name, b, f, e, lim)
            if k and (lim > 0).any():
                r = float((e[lim > 0] / lim[lim > 0]).max())
                if r >= worst:
                    worst, wb = r, float(lim[lim > 0][np.argmax(e[lim > 0] / lim[lim > 0])])
    measured('vc_f0_candidates_f32 %s cost' % name, worst * wb, wb)


@pytest.mark.parametrize('name', list(Cs.YIN_CONFIGS))
def test_yin_and_candidates_per_configuration(name):
    """A ragged batch (lengths 0, 1, hop - 1, hop, G hop - 1, G hop, G hop + 1 and a longer one; ld > max_len; max_frames
    more than a tile beyond the last frame) against the float64 definition; every row alone in tight buffers; the two
    kernels' aperiodicity bit for bit; lens = NULL."""
    poison_gpu_state()
    W, hop, tau_min, tau_max = Cs.YIN_CONFIGS[name]
    rows = Cs.yin_rows(name)
    n_cand = Cs.YIN_NCAND[name]
    res = twice(lambda: run_yin(name, rows), 'vc_f0_yin_f32 ' + name)
    check_yin_rows(name, res, rows)
    cand = twice(lambda: run_cand(name, rows, n_cand), 'vc_f0_candidates_f32 ' + name)
    check_cand_rows(name, cand, rows, n_cand)
    assert np.array_equal(cand['ap'], res['ap']), 'aperiodicity of the two kernels'
    for b, r in enumerate(rows):
        F = 1 + len(r) // hop
        one, onec = run_yin(name, [r], dirty=False), run_cand(name, [r], n_cand, dirty=False)
        for k in ('f0', 'ap'):
            assert np.array_equal(one[k][0, :F], res[k][b, :F]), (name, b, k)
        for k in ('f0', 'pitch', 'cost', 'n', 'ap'):
            assert np.array_equal(onec[k][0, :F], cand[k][b, :F]), (name, b, k)
    # lens = NULL: every row is max_len long (two whole tones, the slack of the stride still NaN)
    full = [Cs.tone(name, len(rows[-1]), ph) for ph in (0.3, 1.7)]
    a, b = run_yin(name, full, null_lens=True), run_yin(name, full)
    ac, bc = run_cand(name, full, n_cand, null_lens=True), run_cand(name, full, n_cand)
    assert all(np.array_equal(a[k], b[k]) for k in a) and all(np.array_equal(ac[k], bc[k]) for k in ac)
    assert (f32(a['f0']) > 0).any()


def test_candidates_keep_the_lowest_in_ascending_lag():
    """More local minima than n_cand: the n_cand lowest of the float64 selection, ascending; a ceiling below every d':
    no candidate in any frame."""
    poison_gpu_state()
    c = Cs.MANY
    cfg = (c['W'], c['hop'], c['tau_min'], c['tau_max'])
    x = Cs.many_minima_signal()
    for n_cand in (1, 2, 15):
        ref = Cs.many_minima_reference(n_cand)
        res = twice(lambda: run_cand(None, [x], n_cand, cfg=cfg), 'many minima')
        f0, n = f32(res['f0'])[0], res['n'][0]
        for f in range(Cs.MANY_KEEP.start, Cs.MANY_KEEP.stop):
            assert n[f] == n_cand
            lag = Cs.SR / f0[f].astype(np.float64)
            assert (np.abs(lag - ref['lag'][f]) <= 0.5 + 4 * EPS * lag).all(), (n_cand, f, lag, ref['lag'][f])
            assert (np.diff(f0[f]) < 0).all()
    for name in Cs.NO_CAND_CONFIGS:
        row = Cs.yin_rows(name)[-1]
        res = twice(lambda: run_cand(name, [row], 2, ceiling=Cs.NO_CAND_CEILING), 'low ceiling')
        assert (res['n'] == 0).all() and (res['f0'] == 0).all() and (res['pitch'] == 0).all() and (res['cost'] == ONE).all()
        assert (f32(res['ap'])[0, :1 + len(row) // Cs.YIN_CONFIGS[name][1]] > Cs.NO_CAND_CEILING).all()


def test_candidates_tie_takes_the_smaller_lag():
    """Integers of period 12 with W = 48: every d is an integer below 2^24 and d' is exactly zero at lags 12, 24 and 36, so the
    n_cand lowest are a tie that the smaller lags win.  Every operation behind cost and f0 is then one correctly rounded
    float32 operation on exact inputs: the float32 restatement bit for bit."""
    poison_gpu_state()
    t = Cs.TIE
    cfg = (t['W'], t['hop'], t['tau_min'], t['tau_max'])
    x = Cs.tie_signal()
    keep = Cs.tie_interior_frames()
    for n_cand, lags in ((1, [12]), (2, [12, 24]), (3, [12, 24, 36])):
        ref = fr.candidates(x, Cs.SR, t['hop'], t['W'], t['tau_min'], t['tau_max'], n_cand, 1.0, np.float32)
        res = twice(lambda: run_cand(None, [x], n_cand, cfg=cfg), 'tie')
        assert (res['n'][0][keep] == n_cand).all()
        assert (ref['lag'][keep] == lags).all()
        assert (res['cost'][0][keep] == 0).all()
        assert np.array_equal(res['f0'][0][keep], ref['f0'][keep].view(np.int32)), n_cand
        assert (np.abs(Cs.SR / f32(res['f0'])[0][keep].astype(np.float64) - np.array(lags)) <= 0.5).all()


def test_candidates_on_a_plateau_take_its_left_end():
    """d'(1) == d'(2) exactly (score_kernels_cases.PLATEAU): a candidate needs d'(tau) < d'(tau - 1) and d'(tau) <=
    d'(tau + 1), so lag 1 is one and lag 2 is not; with lags 4 and 6 the frame has exactly three."""
    poison_gpu_state()
    c = Cs.PLATEAU
    cfg = (c['W'], c['hop'], c['tau_min'], c['tau_max'])
    x = Cs.plateau_signal()
    ref = fr.candidates(x, Cs.SR, c['hop'], c['W'], c['tau_min'], c['tau_max'], c['n_cand'], c['ceiling'], np.float32)
    res = twice(lambda: run_cand(None, [x], c['n_cand'], ceiling=c['ceiling'], cfg=cfg), 'plateau')
    f = c['frame']
    assert res['n'][0, f] == 3
    lag = Cs.SR / f32(res['f0'])[0, f].astype(np.float64)
    assert (np.abs(lag - np.array(c['lags'])) <= 0.5 + 4 * EPS * lag).all(), lag
    assert np.array_equal(res['cost'][0, f], ref['cost'][f].view(np.int32)) and f32(res['cost'])[0, f].tolist() == [1.0, 0.0, float(np.float32(24) / np.float32(19))]
    four = run_cand(None, [x], 4, ceiling=c['ceiling'], cfg=cfg)         # room for a fourth: there is none
    assert four['n'][0, f] == 3 and np.array_equal(four['f0'][0, f, :3], res['f0'][0, f])


def test_yin_and_candidates_refuse_beyond_their_limits():
    poison_gpu_state()
    lib, st = _lib(), _st()
    wav = dev(np.zeros((1, 4096), np.float32))
    outs = [Buf(4096 * 16) for _ in range(4)]
    n = Buf(4096, 'i')

    def yin(W=512, hop=80, tau_max=267, max_frames=52):
        return lib.vc_f0_yin_f32(ptr(wav), None, 1, 4096, 4096, Cs.SR, hop, W, 40, tau_max, 0.15, outs[0].ptr(), outs[1].ptr(), max_frames, st)

    def cand(W=512, hop=80, tau_max=267, max_frames=52, n_cand=15):
        return lib.vc_f0_candidates_f32(ptr(wav), None, 1, 4096, 4096, Cs.SR, hop, W, 40, tau_max, 1.0, n_cand, outs[0].ptr(), outs[1].ptr(),
                                        outs[2].ptr(), n.ptr(), outs[3].ptr(), max_frames, st)

    for fn in (yin, cand):
        _refused(fn(tau_max=1023), VC_ERR_UNSUPPORTED, 'tau_max')
        _refused(fn(W=2049), VC_ERR_UNSUPPORTED, 'frame_length')
        _refused(fn(max_frames=51), VC_ERR_INVALID, 'max_frames 51 is less than')
    _refused(cand(n_cand=16), VC_ERR_UNSUPPORTED, 'n_cand')
    _refused(cand(n_cand=0), VC_ERR_INVALID, 'n_cand')
    assert all(o.untouched() for o in outs) and n.untouched()
    _ok(yin(tau_max=1022, W=2048))
    _ok(cand(n_cand=15, tau_max=1022, W=2048))
    assert all(o.bands_ok() for o in outs) and n.bands_ok()


# ================================================================================================ F0 metrics
def run_metrics(fa, fb, paths, dirty=True):
    """fa, fb: lists of tracks; paths: None or list of [n, 2] arrays."""
    B = len(fa)
    la, lb = [len(x) for x in fa], [len(x) for x in fb]
    max_a, max_b = (max(la) + 3, max(lb) + 11) if dirty else (max(la), max(lb))
    A, Bt = dev(padded(fa, max_a, np.nan if dirty else 0.0)), dev(padded(fb, max_b, np.nan if dirty else 0.0))
    d_path = d_plen = None
    max_path = 0
    if paths is not None:
        pl = [len(p) for p in paths]
        max_path = max(max(pl), 1) + (7 if dirty else 0)
        d_path = dev(padded([np.asarray(p, np.int32).reshape(-1, 2) for p in paths], max_path, IFILL if dirty else 0, np.int32, tail=(2,)))
        d_plen = i32(pl)
    counts, values = Buf(B * 3, 'i'), Buf(B * 4)
    d_la, d_lb = i32(la), i32(lb)
    _ok(_lib().vc_f0_metrics_f32(ptr(A), ptr(Bt), ptr(d_la), ptr(d_lb), B, max_a, max_b, ptr(d_path), ptr(d_plen), max_path, counts.ptr(),
                                 values.ptr(), _st()))
    return dict(counts=counts.bits((B, 3)), values=values.bits((B, 4)))


VALUE_KEYS = ('vuv_error', 'f0_rmse_cents', 'f0_rmse_hz', 'logf0_corr')


def check_metrics(res, b, ref, what):
    assert res['counts'][b].tolist() == [ref['n_cells'], ref['n_both_voiced'], ref['n_vuv_mismatch']], (what, res['counts'][b], ref)
    worst = 0.0
    for k, name in enumerate(VALUE_KEYS):
        got, want = float(f32(res['values'])[b, k]), float(ref[name])
        if np.isnan(want):
            assert np.isnan(got), (what, name, got)
            continue
        bound = Cs.metrics_bound(want, max(ref['n_cells'], 1))
        assert abs(got - want) <= bound, (what, name, got, want, bound)
        worst = max(worst, abs(got - want) / bound)
    return worst


def _track(rng, n, p_voiced=0.7):
    return np.where(rng.rand(n) < p_voiced, rng.uniform(80.0, 300.0, n), 0.0).astype(np.float32)


def test_f0_metrics_against_float64():
    """Cells 255, 256, 257 and 1,000 with the path NULL and given (max_path > path_len, 0x7fffffff behind it, NaN behind the
    tracks); cells outside either track skipped and counted nowhere."""
    poison_gpu_state()
    rng = np.random.RandomState(8)
    fa = [_track(rng, n + (5 if k % 2 else 0)) for k, n in enumerate(Cs.METRIC_CELLS)]
    fb = [_track(rng, n + (0 if k % 2 else 4)) for k, n in enumerate(Cs.METRIC_CELLS)]
    fb = [np.where(b > 0, b * rng.uniform(0.9, 1.1, len(b)), 0).astype(np.float32) for b in fb]
    worst = 0.0
    res = twice(lambda: run_metrics(fa, fb, None), 'vc_f0_metrics_f32 diagonal')
    for b in range(len(fa)):
        assert min(len(fa[b]), len(fb[b])) == Cs.METRIC_CELLS[b]
        worst = max(worst, check_metrics(res, b, fr.metrics(fa[b], fb[b], len(fa[b]), len(fb[b])), 'diagonal %d' % b))
        assert np.array_equal(run_metrics([fa[b]], [fb[b]], None, dirty=False)['values'][0], res['values'][b])
    paths = []
    for b, n in enumerate(Cs.METRIC_CELLS):
        p = np.stack([rng.randint(0, len(fa[b]), n + 20), rng.randint(0, len(fb[b]), n + 20)], 1)
        bad = rng.permutation(n + 20)[:20]                               # twenty cells outside either track
        p[bad[:5], 0], p[bad[5:10], 0] = -1, len(fa[b])
        p[bad[10:15], 1], p[bad[15:], 1] = -3, len(fb[b]) + 2
        paths.append(p)
    res = twice(lambda: run_metrics(fa, fb, paths), 'vc_f0_metrics_f32 path')
    for b in range(len(fa)):
        ref = fr.metrics(fa[b], fb[b], len(fa[b]), len(fb[b]), paths[b])
        assert ref['n_cells'] == Cs.METRIC_CELLS[b]
        worst = max(worst, check_metrics(res, b, ref, 'path %d' % b))
        alone = run_metrics([fa[b]], [fb[b]], [paths[b]], dirty=False)
        assert np.array_equal(alone['values'][0], res['values'][b]) and np.array_equal(alone['counts'][0], res['counts'][b])
    measured('vc_f0_metrics_f32 worst figure', worst, 1.0)


def test_f0_metrics_undefined_figures_are_nan():
    poison_gpu_state()
    v = np.float32
    fa = [np.array([100, 0, 120], v), np.array([100, 0, 0], v), np.array([100, 100, 100, 0], v), np.array([0, 0], v), np.array([90, 110], v)]
    fb = [np.array([110, 0, 130], v), np.array([105, 50, 0], v), np.array([90, 110, 120, 0], v), np.array([0, 0, 0], v), np.array([95, 100], v)]
    paths = [np.zeros((0, 2), np.int32),                                  # no cell: zero counts and four NaNs
             np.array([[0, 0], [1, 1], [2, 2]]),                          # one cell voiced on both sides
             np.array([[0, 0], [1, 1], [2, 2], [3, 3]]),                  # a constant track on side a
             np.array([[0, 0], [1, 2]]),                                  # no voiced cell
             np.array([[5, 0], [0, 7], [-1, -1]])]                        # every cell outside: as no cell
    res = twice(lambda: run_metrics(fa, fb, paths), 'undefined figures')
    vals = f32(res['values'])
    for b in range(5):
        check_metrics(res, b, fr.metrics(fa[b], fb[b], len(fa[b]), len(fb[b]), paths[b]), 'case %d' % b)
    assert res['counts'][0].tolist() == [0, 0, 0] and np.isnan(vals[0]).all()
    assert res['counts'][4].tolist() == [0, 0, 0] and np.isnan(vals[4]).all()
    assert np.isnan(vals[1, 3]) and np.isfinite(vals[1, :3]).all() and res['counts'][1].tolist() == [3, 1, 1]
    assert np.isnan(vals[2, 3]) and np.isfinite(vals[2, :3]).all() and res['counts'][2, 1] == 3
    assert vals[3, 0] == 0 and np.isnan(vals[3, 1:]).all()


# ================================================================================================ frame energy
def run_energy(W, hop, rows, dirty=True, null_lens=False):
    wav, d_lens, lens, max_len, ld = _wave_batch(rows, dirty, null_lens)
    B = len(rows)
    max_frames = 1 + max_len // hop + ((Cs.energy_tile(W, hop) + 3) if dirty else 0)
    out = Buf(B * max_frames)
    _ok(_lib().vc_frame_energy_f32(ptr(wav), ptr(d_lens), B, max_len, ld, hop, W, out.ptr(), max_frames, _st()))
    return dict(e=out.bits((B, max_frames)))


@pytest.mark.parametrize('W,hop', Cs.ENERGY_CONFIGS)
def test_frame_energy_against_float64(W, hop):
    poison_gpu_state()
    assert _lib().vc_frame_energy_tile(hop, W) == Cs.energy_tile(W, hop)
    rows = Cs.energy_rows(W, hop)
    res = twice(lambda: run_energy(W, hop, rows), 'vc_frame_energy_f32')
    worst = 0.0
    for b, r in enumerate(rows):
        F = 1 + len(r) // hop
        want = ar.frame_energy(r, hop, W)
        got = f32(res['e'])[b]
        assert (res['e'][b, F:] == 0).all(), (b, 'frames past the utterance')
        err = np.abs(got[:F].astype(np.float64) - want)
        assert (err <= Cs.energy_bound(W) * want).all(), (b, err.max())
        if (want > 0).any():
            worst = max(worst, float((err[want > 0] / want[want > 0]).max()))
        assert np.array_equal(run_energy(W, hop, [r], dirty=False)['e'][0, :F], res['e'][b, :F]), b
    measured('vc_frame_energy_f32 W%d hop%d relative' % (W, hop), worst, Cs.energy_bound(W))
    full = [rows[-1], rows[-1][::-1].copy()]
    a, c = run_energy(W, hop, full, null_lens=True), run_energy(W, hop, full)
    assert np.array_equal(a['e'], c['e'])


# ================================================================================================ activity mask
def run_mask(energies, f0s, frames, mode, ratio, max_gap, min_run, dirty=True, max_frames=None):
    B = len(frames)
    max_frames = max_frames or (min(max(frames) + 37, 16384) if dirty else max(frames))
    fill = np.nan if dirty else 0.0
    E = None if energies is None else dev(padded(energies, max_frames, fill))
    P = None if f0s is None else dev(padded(f0s, max_frames, fill))
    out = Buf(B * max_frames, 'b')
    d_frames = i32(frames)
    _ok(_lib().vc_activity_mask(ptr(E), ptr(P), ptr(d_frames), B, max_frames, mode, ratio, max_gap, min_run, out.ptr(), _st()))
    m = out.bits((B, max_frames))
    assert ((m == 0) | (m == 1)).all(), 'every mask byte is written with 0 or 1'
    return dict(mask=m)


def check_mask(res, raws, max_gap, min_run, what):
    for b, raw in enumerate(raws):
        F = len(raw)
        want = ar.smooth(raw, max_gap, min_run)
        got = res['mask'][b]
        assert np.array_equal(got[:F].astype(bool), want), (what, b, F, np.nonzero(got[:F].astype(bool) != want)[0][:10])
        assert (got[F:] == 0).all(), (what, b)


@pytest.mark.parametrize('F', Cs.MASK_FRAMES)
def test_activity_mask_is_exact_around_the_lane_boundaries(F):
    """Gaps of max_gap and max_gap + 1 and runs of min_run - 1 and min_run over a lane boundary and at both ends, for
    every number of frames per lane; max_gap >= F, min_run > F; modes 1 (f0 = NULL), 2 (energy = NULL) and 3."""
    poison_gpu_state()
    rng = np.random.RandomState(F)
    raws = [Cs.lane_pattern(F), Cs.mirrored(Cs.lane_pattern(F))] + [rng.rand(F) < p for p in (0.5, 0.9, 0.1)]
    es = [Cs.energies_of(r, rng) for r in raws]
    for r, e in zip(raws, es):
        assert np.array_equal(Cs.raw_decision(e, 1e-4), r)
    for max_gap, min_run in ((Cs.MAX_GAP, Cs.MIN_RUN), (0, 0), (0, 1), (1, 2), (F, 0), (F + 5, F + 1), (0, F + 1), (0, F), (16, 31)):
        what = 'F %d gap %d run %d' % (F, max_gap, min_run)
        res = twice(lambda: run_mask(es, None, [F] * len(raws), 1, 1e-4, max_gap, min_run), what)
        check_mask(res, raws, max_gap, min_run, what)
        if (max_gap, min_run) in ((Cs.MAX_GAP, Cs.MIN_RUN), (16, 31)):
            for b in (0, 1, 2):
                one = run_mask([es[b]], None, [F], 1, 1e-4, max_gap, min_run, dirty=False)
                assert np.array_equal(one['mask'][0], res['mask'][b, :F]), (what, b)
    f0s = [np.where(r, 120.0, np.where(rng.rand(F) < 0.5, 0.0, -50.0)).astype(np.float32) for r in raws]
    res = twice(lambda: run_mask(None, f0s, [F] * len(raws), 2, 0.0, Cs.MAX_GAP, Cs.MIN_RUN), 'mode 2')
    check_mask(res, raws, Cs.MAX_GAP, Cs.MIN_RUN, 'mode 2, F %d' % F)
    voiced = [rng.rand(F) < 0.8 for _ in raws]
    f0s = [np.where(v, 120.0, 0.0).astype(np.float32) for v in voiced]
    res = twice(lambda: run_mask(es, f0s, [F] * len(raws), 3, 1e-4, Cs.MAX_GAP, Cs.MIN_RUN), 'mode 3')
    check_mask(res, [r & v for r, v in zip(raws, voiced)], Cs.MAX_GAP, Cs.MIN_RUN, 'mode 3, F %d' % F)


def test_activity_mask_ragged_threshold_and_refusals():
    """One ragged batch over every frame count (NaN energies behind each row's frames); an energy equal to the threshold
    is inactive (the compare is strict), the next float32 above it active; all-zero energy: no active frame; frame counts
    clamped to [1, max_frames]; ratio outside (0, 1) refused."""
    poison_gpu_state()
    rng = np.random.RandomState(2)
    raws = [Cs.lane_pattern(F) for F in Cs.MASK_FRAMES]
    es = [Cs.energies_of(r, rng) for r in raws]
    raws = [Cs.raw_decision(e, 1e-4) for e in es]                        # (a row without an active frame has no 1.0 in it)
    res = twice(lambda: run_mask(es, None, list(Cs.MASK_FRAMES), 1, 1e-4, Cs.MAX_GAP, Cs.MIN_RUN, max_frames=16384), 'ragged')
    check_mask(res, raws, Cs.MAX_GAP, Cs.MIN_RUN, 'ragged')
    up = np.nextafter(np.float32(0.25), np.float32(1))
    e = np.array([1.0, 0.25, up, 0.0, 0.25, up, 0.5], np.float32)
    res = twice(lambda: run_mask([e, np.zeros(7, np.float32)], None, [7, 7], 1, 0.25, 0, 0), 'threshold')
    assert res['mask'][0, :7].tolist() == [1, 0, 1, 0, 0, 1, 1] and (res['mask'][1] == 0).all()
    res = run_mask([e, e, e], None, [0, -4, 99], 1, 0.25, 0, 0, dirty=False, max_frames=7)
    assert res['mask'][0].tolist() == [1, 0, 0, 0, 0, 0, 0] and res['mask'][1].tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert res['mask'][2].tolist() == [1, 0, 1, 0, 0, 1, 1]
    lib, st = _lib(), _st()
    E, n, out = dev(e), i32([7]), Buf(7, 'b')
    for ratio in (0.0, 1.0, -0.5, float('nan')):
        _refused(lib.vc_activity_mask(ptr(E), None, ptr(n), 1, 7, 1, ratio, 0, 0, out.ptr(), st), VC_ERR_INVALID, 'ratio')
    _refused(lib.vc_activity_mask(ptr(E), None, ptr(n), 1, 7, 2, 0.5, 0, 0, out.ptr(), st), VC_ERR_INVALID, 'd_f0')
    _refused(lib.vc_activity_mask(None, ptr(E), ptr(n), 1, 7, 3, 0.5, 0, 0, out.ptr(), st), VC_ERR_INVALID, 'd_energy')
    _refused(lib.vc_activity_mask(ptr(E), None, ptr(n), 1, 16385, 1, 0.5, 0, 0, out.ptr(), st), VC_ERR_UNSUPPORTED, 'max_frames')
    assert out.untouched()


# ================================================================================================ compaction
def run_compact(masks_a, masks_b=None, dirty=True):
    B = len(masks_a)
    Fa = [len(m) for m in masks_a]
    max_a = max(Fa) + (6 if dirty else 0)
    A = dev(padded([np.asarray(m, np.uint8) for m in masks_a], max_a, 1 if dirty else 0, np.uint8))      # active bytes behind the frames
    Bm = fb = None
    max_b = 0
    if masks_b is not None:
        Fb = [len(m) for m in masks_b]
        max_b = max(Fb) + (3 if dirty else 0)
        Bm, fb = dev(padded([np.asarray(m, np.uint8) for m in masks_b], max_b, 1 if dirty else 0, np.uint8)), i32(Fb)
    max_int = (max_a + 1) // 2
    index, iv = Buf(B * max_a, 'i'), Buf(B * max_int * 2, 'i')
    na, nk, ni = Buf(B, 'i'), Buf(B, 'i'), Buf(B, 'i')
    fa = i32(Fa)
    _ok(_lib().vc_mask_compact(ptr(A), ptr(fa), max_a, ptr(Bm), ptr(fb), max_b, B, index.ptr(), na.ptr(), nk.ptr(), iv.ptr(), ni.ptr(), _st()))
    return dict(index=index.bits((B, max_a)), intervals=iv.bits((B, max_int, 2)), n_active=na.bits(), n_kept=nk.bits(), n_intervals=ni.bits())


def check_compact(res, b, ref, what):
    k, n = ref['n_kept'], len(ref['intervals'])
    assert (int(res['n_active'][b]), int(res['n_kept'][b]), int(res['n_intervals'][b])) == (ref['n_active'], k, n), what
    assert np.array_equal(res['index'][b, :k], ref['index']) and (res['index'][b, k:] == -1).all(), what
    assert np.array_equal(res['intervals'][b, :n], ref['intervals']) and (res['intervals'][b, n:] == -1).all(), what


def test_mask_compact_one_and_two_masks():
    poison_gpu_state()
    rng = np.random.RandomState(4)
    for F in (1, 7, 1025, 2049, 16377):
        alt = (np.arange(F) % 2 == 0)                                   # 1010...1: (F + 1) / 2 intervals
        masks = [alt, np.zeros(F, bool), np.ones(F, bool), rng.rand(F) < 0.5, ~alt, (rng.rand(max(F - 3, 1)) < 0.9)]
        res = twice(lambda: run_compact(masks), 'vc_mask_compact')
        for b, m in enumerate(masks):
            check_compact(res, b, ar.compact(m), 'F %d mask %d' % (F, b))
            check_compact(run_compact([m], dirty=False), 0, ar.compact(m), 'F %d mask %d alone' % (F, b))
        one = run_compact([alt], dirty=False)                            # tight: the intervals fill the buffer to its last slot
        assert int(one['n_intervals'][0]) == (F + 1) // 2 == one['intervals'].shape[1]
        assert one['intervals'][0, -1].tolist() == [F - 1, F]
        assert int(res['n_kept'][1]) == F and int(res['n_active'][1]) == 0 and int(res['n_intervals'][1]) == 0      # keep-all fallback
        others = [rng.rand(n) < 0.6 for n in (F + 4, max(F - 2, 1), F, max(F // 2, 1), F + 1, F)]
        res = twice(lambda: run_compact(masks, others), 'vc_mask_compact two masks')
        for b, (m, o) in enumerate(zip(masks, others)):
            check_compact(res, b, ar.compact(m, o), 'F %d masks %d' % (F, b))


def test_compact_rows_gathers_and_zero_fills():
    poison_gpu_state()
    lib, st = _lib(), _st()
    rng = np.random.RandomState(6)
    src_frames, index_frames, B = 9, 12, 5
    n_kept = [-2, 0, 7, 15, 12]
    for n_cols in (1, 3, 80, 4096):
        src = rng.standard_normal((B, src_frames, n_cols)).astype(np.float32)
        index = np.full((B, index_frames), IFILL, np.int32)
        for b in range(B):
            k = min(max(n_kept[b], 0), index_frames)
            index[b, :k] = rng.randint(0, src_frames, k)
            index[b, :k][::4] = [-1, src_frames, src_frames + 100, -7][b % 4]      # entries outside the source: zero rows
        d_src, d_index, d_kept = dev(src), dev(index), i32(n_kept)
        for dst_frames in (5, 20):
            def run():
                out = Buf(B * dst_frames * n_cols)
                _ok(lib.vc_compact_rows_f32(ptr(d_src), src_frames, ptr(d_index), index_frames, ptr(d_kept), B, n_cols, out.ptr(), dst_frames, st))
                return dict(dst=out.bits((B, dst_frames, n_cols)))
            got = f32(twice(run, 'vc_compact_rows_f32')['dst'])
            want = np.zeros((B, dst_frames, n_cols), np.float32)
            for b in range(B):
                for k in range(min(min(max(n_kept[b], 0), index_frames), dst_frames)):
                    if 0 <= index[b, k] < src_frames:
                        want[b, k] = src[b, index[b, k]]
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n_cols, dst_frames)
    out = Buf(16)
    _refused(lib.vc_compact_rows_f32(ptr(d_src), src_frames, ptr(d_index), index_frames, ptr(d_kept), B, 4097, out.ptr(), 1, st),
             VC_ERR_UNSUPPORTED, 'n_cols')
    assert out.untouched()


def test_path_map_maps_clamps_and_marks():
    """d_path_in NULL: the cells (p, p); a cell outside [0, max_a) x [0, max_b): (-1, -1); rows from path_len on: (-1, -1);
    a path_len above max_path is clamped to it, one below zero to zero."""
    poison_gpu_state()
    lib, st = _lib(), _st()
    rng = np.random.RandomState(9)
    B, max_a, max_b, max_path = 5, 300, 270, 300 + 270 - 1
    ia, ib = rng.randint(0, 5000, (B, max_a)).astype(np.int32), rng.randint(0, 5000, (B, max_b)).astype(np.int32)
    plen = [0, 257, max_path, max_path + 50, -3]
    path = np.full((B, max_path, 2), IFILL, np.int32)
    for b in range(B):
        n = min(max(plen[b], 0), max_path)
        path[b, :n, 0], path[b, :n, 1] = rng.randint(0, max_a, n), rng.randint(0, max_b, n)
        path[b, :n:7, 0] = [-1, max_a, max_a + 3][b % 3]
        path[b, 3:n:11, 1] = [max_b, -2, IFILL][b % 3]
    d_ia, d_ib, d_len = dev(ia), dev(ib), i32(plen)
    for given in (True, False):
        d_in = dev(path) if given else None

        def run():
            out = Buf(B * max_path * 2, 'i')
            _ok(lib.vc_path_map(ptr(d_in), ptr(d_len), B, max_path, ptr(d_ia), max_a, ptr(d_ib), max_b, out.ptr(), st))
            return dict(path=out.bits((B, max_path, 2)))
        got = twice(run, 'vc_path_map')['path']
        want = np.full((B, max_path, 2), -1, np.int32)
        for b in range(B):
            for p in range(min(max(plen[b], 0), max_path)):
                i, j = (path[b, p] if given else (p, p))
                if 0 <= i < max_a and 0 <= j < max_b:
                    want[b, p] = ia[b, i], ib[b, j]
        assert np.array_equal(got, want), given


# ================================================================================================ gain
def run_gain(rows, masks, n_active, hop, target, dirty=True):
    wav, d_lens, lens, max_len, ld = _wave_batch(rows, dirty)
    B = len(rows)
    max_frames = 1 + max_len // hop + (4 if dirty else 0)
    M = dev(padded([np.asarray(m, np.uint8) for m in masks], max_frames, 1 if dirty else 0, np.uint8))
    gain, out = Buf(B), Buf(B * max_len)
    d_act = i32(n_active)
    lib, st = _lib(), _st()
    _ok(lib.vc_speech_gain_f32(ptr(wav), ptr(d_lens), B, max_len, ld, hop, ptr(M), ptr(d_act), max_frames, target, gain.ptr(), st))
    _ok(lib.vc_scale_rows_f32(ptr(wav), ptr(d_lens), B, max_len, ld, gain.ptr(), out.ptr(), st))
    assert gain.bands_ok()
    return dict(gain=gain.bits(), out=out.bits((B, max_len)))


@pytest.mark.parametrize('hop', Cs.GAIN_HOPS)
def test_speech_gain_and_scale_rows(hop):
    """Lengths 0, 1, 1023, 1024, 1025; the sample-to-frame map min((i + hop / 2) / hop, F - 1) at its seams (one active
    frame: exactly its hop samples count); n_active = 0: all samples; all-zero samples: gain 1; rows past len exactly zero."""
    poison_gpu_state()
    rng = np.random.RandomState(hop)
    target = np.float32(0.003)
    rows, masks = [], []
    for n in Cs.GAIN_LENGTHS:
        rows.append((0.1 * rng.standard_normal(n)).astype(np.float32))
        masks.append(rng.rand(1 + n // hop) < 0.5)
    for f in (0, 1, 1025 // hop - 1, 1025 // hop):                      # one active frame: first, second, last but one, last
        rows.append((0.1 * rng.standard_normal(1025)).astype(np.float32))
        m = np.zeros(1 + 1025 // hop, bool)
        m[f] = True
        masks.append(m)
    rows.append((0.1 * rng.standard_normal(1025)).astype(np.float32))
    masks.append(np.zeros(1 + 1025 // hop, bool))                        # n_active = 0: over all samples
    rows.append(np.zeros(700, np.float32))
    masks.append(np.ones(1 + 700 // hop, bool))                          # all-zero samples: gain 1
    n_active = [int(m.sum()) for m in masks]
    res = twice(lambda: run_gain(rows, masks, n_active, hop, float(target)), 'vc_speech_gain_f32')
    gain = f32(res['gain'])
    worst = 0.0
    for b, (x, m) in enumerate(zip(rows, masks)):
        want = ar.speech_gain(x, m, hop, float(target))
        err = abs(float(gain[b]) / want - 1)
        assert err <= Cs.gain_bound(), (b, len(x), gain[b], want)
        worst = max(worst, err)
        out = f32(res['out'])[b]
        assert np.array_equal(out[:len(x)].view(np.int32), (gain[b] * x).view(np.int32)), b
        assert (res['out'][b, len(x):] == 0).all(), (b, 'samples past the utterance')
        one = run_gain([x], [m], [n_active[b]], hop, float(target), dirty=False)
        assert one['gain'][0] == res['gain'][b] and np.array_equal(one['out'][0, :len(x)], res['out'][b, :len(x)]), b
    assert gain[0] == 1 and gain[-1] == 1 and (gain[1:-1] != 1).all()
    measured('vc_speech_gain_f32 hop %d relative' % hop, worst, Cs.gain_bound())
    # the seam by counting: ones, one active frame f -> gain = target exactly when any sample is counted, and the float64
    # sum over |x| = sample index tells WHICH samples were
    x = np.arange(1, 1026, dtype=np.float32)
    F = 1 + 1025 // hop
    for f in (0, 1, F - 2, F - 1):
        m = np.zeros(F, bool)
        m[f] = True
        g = f32(run_gain([x], [m], [1], hop, 1.0, dirty=False)['gain'])[0]
        idx = np.nonzero(Cs.frame_of_sample(np.arange(1025), hop, F) == f)[0]
        assert g == np.float32(len(idx) / x[idx].astype(np.float64).sum()), (hop, f)
