"""MX-FP8 inference of the decoder's filter banks and projection (speech-cloner_amd/mx8.py, csrc/vc_mx8.hip) on the
MI355X: the device quantiser bit for bit against tests/mx8_ref.py, the MFMA lane map with exact integers, both kernel
forms against float64 of the device's own quantised operands, the MX epilogue against the CPU quantiser applied to the
float64 values (independent of the device's rounding decisions), the whole decoder against the float64 oracle, process
isolation from the bf16 path and the public API.

Kernel tolerance (cases 3 and 5).  Stated first from float32 accumulation alone -- (n + 64) 2^-24 sum |a w|, n = taps *
Cin / 64 chained MFMAs -- it failed on the first MI355X run by 2.7x, and a diagnostic run located the difference in the
instruction itself: with ONE filter tap (two MFMAs, an exact epilogue) the error is already 2^-16.5 sum |a w|, unbiased,
with or without e4m3 subnormals in the operands.  v_mfma_scale_f32_32x32x64_f8f6f4 sums its 64 products to ~17 bits
relative to their magnitude sum, not to float32.  The bound is therefore
     |err| <= ( 2^-15 + (n + 4) 2^-24 ) * |s| * sum |a * w|  +  2^-23 |shift|          per output element
(the instruction's own summation, measured worst 2^-16.5 / 2^-17.5 at K = 2 / 32, with 2.8x margin; the float32 chain of
n MFMA results; the epilogue's fma), before relu / pool, which do not increase it; s, shift the folded BatchNorm.

Whole decoder (case 6), end-to-end bound DERIVED before the first GPU run:
  * the MX roundings alone (tests/test_mx8_cpu.py, float64 simulation on 2 seeded windows at the shipped sizes) cost
    y_mel max 6.9e-3 / rms 1.8e-3 and y_stft max 5.2e-3 / rms 1.1e-3;
  * the device rounds the same tensors, but of values that carry the bf16 path's drift, and other windows: x2 for
    the spread, plus the bf16 path's own regression allowance (tests/test_bench_config_gpu.py (R): max 1.5e-2, rms 3e-3):
        max |err| <= 3.0e-2,  rms err <= 7e-3                                                       ... (D)
  * beside it a REGRESSION bound at <= 5x the figures measured on an MI355X: y_mel max 7.1e-3
    / rms 2.0e-3, y_stft max 6.0e-3 / rms 1.2e-3 at 64 and 128 windows  ->  max 2.0e-2, rms 5e-3 ...... (R)
bf16 today (same test, round 2): y_mel max 2.9e-3 / rms 6.1e-4, y_stft max 2.0e-3 / rms 4.2e-4; the bf16 figures of
the same windows are printed beside the mxfp8 ones."""
import json
import os

import numpy as np
import pytest
import torch

import mx8_ref as mx
from conftest import ROOT, poison_gpu_state
from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu

DER_MAX, DER_RMS = 3.0e-2, 7e-3          # (D)
REG_MAX, REG_RMS = 2.0e-2, 5e-3          # (R): measured max 7.1e-3 / rms 2.0e-3: 2.8x / 2.6x
HP = os.path.join(ROOT, 'speech-cloner_amd', 'hp')


@pytest.fixture(scope='module', autouse=True)
def _poison():
    poison_gpu_state()


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------- 1. quantiser
def _sweep(rng):
    rows = []
    rows.append(rng.standard_normal((64, 256)) * np.ldexp(1.0, rng.randint(-40, 40, size=(64, 1))))
    mids = (mx.POS[:-1] + mx.POS[1:]) / 2                      # every midpoint, at scales 2^-3 .. 2^3
    for e in range(-3, 4):
        r = np.zeros(256)
        r[:126], r[126:252] = mids, -mids
        r[252:256] = 448.0
        blocks = r.reshape(8, 32)
        blocks[:, 0] = 448.0                                     # amax 448: scale e exactly
        rows.append(blocks.reshape(1, 256) * 2.0 ** e)
    sub = np.arange(256) * 2.0 ** -11                          # e4m3 subnormals and their midpoints (scale 0 blocks)
    sub = sub.reshape(8, 32)
    sub[:, 31] = 448.0
    rows.append(sub.reshape(1, 256))
    z = np.zeros((1, 256))
    z[0, 32:64] = -0.0
    z[0, 64:96] = rng.standard_normal(32)
    z[0, 64:80] = -0.0
    rows.append(z)
    edge = []                                                   # amax on and around powers of two and 448 * 2^k
    for k in range(-10, 11):
        for v in (2.0 ** k, 448.0 * 2.0 ** k, 1.75 * 2.0 ** k):
            for a in (np.nextafter(np.float32(v), np.float32(0)), np.float32(v), np.nextafter(np.float32(v), np.float32(1e30))):
                b = rng.uniform(-1, 1, 32) * float(a) * 0.9
                b[rng.randint(32)] = a
                edge.append(b)
    edge = np.array(edge)
    edge = edge[:edge.shape[0] // 8 * 8].reshape(-1, 256)
    rows.append(edge)
    return np.concatenate(rows).astype(np.float32)


@pytest.mark.parametrize('src', ['f32', 'bf16'])
def test_device_quantiser_matches_cpu_bit_for_bit(src):
    import mx8
    x = torch.from_numpy(_sweep(np.random.RandomState(3))).cuda()
    if src == 'bf16':
        x = x.bfloat16()
    M, C = x.shape
    codes, scales = mx8.quantize(x, M, C)
    rc, rs = mx.quantize(_np(x.float()))
    assert np.array_equal(_np(scales), rs), np.argwhere(_np(scales) != rs)[:8]
    bad = np.argwhere(_np(codes) != rc)
    assert bad.size == 0, [(tuple(i), hex(_np(codes)[tuple(i)]), hex(rc[tuple(i)]), float(_np(x.float())[tuple(i)])) for i in bad[:8]]
    # a row stride: the same values read from the left half of a wider buffer
    wide = torch.zeros((M, C + 64), dtype=x.dtype, device='cuda')
    wide[:, :C] = x
    c2, s2 = mx8.quantize(wide, M, C, ldx=C + 64)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


# ------------------------------------------------------------------------------------------------------ 2. lane map
def test_lane_map_exact_small_integers():
    """One tile (128 frames, one window, taps 1, 2 K steps of 64): small-integer e4m3 elements, an asymmetric weight
    matrix and a different scale per 32-block -- every product and sum is exact in float32, so the result is exact."""
    import mx8
    import _vc
    rng = np.random.RandomState(11)
    vals = np.array([0x00, 0x38, 0x40, 0x44, 0x48, 0xB8, 0xC0, 0xC4], np.uint8)    # 0 1 2 3 4 -1 -2 -3
    M, Cin = 128, 128
    xc = vals[rng.randint(0, 8, (M, Cin))]
    xs = rng.randint(125, 130, (M, Cin // 32)).astype(np.uint8)
    wc = vals[rng.randint(0, 8, (128, Cin))]
    wc[np.arange(128), np.arange(128) % Cin] = 0x48                          # asymmetric: W != W^T by construction
    ws = rng.randint(124, 131, (128, Cin // 32)).astype(np.uint8)
    X = mx8.MxTensor(torch.from_numpy(xc).cuda().view(1, M, Cin), torch.from_numpy(xs).cuda().view(1, M, Cin // 32))
    packed = (torch.from_numpy(wc).cuda(), torch.from_numpy(ws).cuda())
    one = torch.ones(128, device='cuda')
    zero = torch.zeros(128, device='cuda')
    y = mx8.conv(X, packed, 1, 128, one, zero, _vc.ACT_NONE, out_mode=_vc.MX8_OUT_F32)
    ref = mx.dequantize(xc, xs) @ mx.dequantize(wc, ws).T
    assert np.array_equal(_np(y)[0], ref), np.abs(_np(y)[0] - ref).max()


# ---------------------------------------------------------------------------------------- 3./4. bank kernel
def _acc_tol(n_mfma):
    """relative tolerance against sum |a w| of a chain of n_mfma scaled MFMAs (module docstring)"""
    return 2.0 ** -15 + (n_mfma + 4) * 2.0 ** -24


def _bank_case(K, Cin, N=3, T=400, seed=0):
    import mx8
    import _vc
    rng = np.random.RandomState(seed)
    x = torch.from_numpy(rng.standard_normal((N, T, Cin)).astype(np.float32)).cuda().bfloat16()
    kern = [torch.from_numpy(rng.uniform(-0.06, 0.06, (k, Cin, 128)).astype(np.float32)).cuda() for k in range(1, K + 1)]
    packed = [mx8.pack_kernel(k) for k in kern]
    s = torch.from_numpy(rng.uniform(0.5, 2.0, 128 * K).astype(np.float32)).cuda()
    sh = torch.from_numpy(rng.uniform(-0.3, 0.3, 128 * K).astype(np.float32)).cuda()
    y32 = mx8.bank(x, packed, K, s, sh, out_mode=_vc.MX8_OUT_F32)
    ymx = mx8.bank(x, packed, K, s, sh)
    # float64 of the device's own operands
    xq, xs = mx8.quantize(x.view(N * T, Cin), N * T, Cin)
    xd = torch.from_numpy(mx.dequantize(_np(xq), _np(xs)).reshape(N, T, Cin))
    pre, bnd = [], []
    for k, (w, ws) in zip(range(1, K + 1), packed):
        wd = torch.from_numpy(mx.dequantize(_np(w), _np(ws)).T.reshape(k, Cin, 128).copy())
        pre.append(mo.conv1d(xd, wd))
        bnd.append(mo.conv1d(xd.abs(), wd.abs()) * _acc_tol(k * Cin // 64))
    sd, shd = torch.from_numpy(_np(s)).double(), torch.from_numpy(_np(sh)).double()
    pre = torch.cat(pre, -1) * sd + shd
    tol = torch.cat(bnd, -1) * sd.abs() + shd.abs() * 2.0 ** -23
    ref = mo.max_pool_2_same(torch.relu(pre))
    tol = mo.max_pool_2_same(tol)
    return y32, ymx, ref.numpy(), tol.numpy()


def test_scaled_mfma_sums_its_products_to_about_17_bits():
    """Pins the instruction property the kernel tolerance rests on (module docstring; tools/mx8_mfma_accumulation.py):
    the width-1 filter of a raw bank launch (no BN / relu / pool, float32 out) is two MFMAs and an exact epilogue, so
    its error against float64 of the device's operands is the instruction's own.  Measured 2^-16.5 sum |a w|: coarser
    than a float32 sum of two terms (2^-23) and inside the 2^-15 the tolerance allows."""
    import mx8
    import _vc
    rng = np.random.RandomState(0)
    N, T, Cin = 3, 400, 128
    x = torch.from_numpy(rng.standard_normal((N, T, Cin)).astype(np.float32)).cuda().bfloat16()
    kern = [torch.from_numpy(rng.uniform(-0.06, 0.06, (k, Cin, 128)).astype(np.float32)).cuda() for k in (1, 2)]
    packed = [mx8.pack_kernel(k) for k in kern]
    xq, xs = mx8.quantize(x.view(N * T, Cin), N * T, Cin)
    out = torch.empty((N, T, 256), device='cuda')
    mx8._launch(xq, xs, N * T, T, Cin, mx8.bank_groups(packed, 2, Cin), torch.ones(256, device='cuda'),
                torch.zeros(256, device='cuda'), _vc.ACT_NONE, 0, _vc.MX8_OUT_F32, 256, out)
    xd = torch.from_numpy(mx.dequantize(_np(xq), _np(xs)).reshape(N, T, Cin))
    wd = torch.from_numpy(mx.dequantize(_np(packed[0][0]), _np(packed[0][1])).T.reshape(1, Cin, 128).copy())
    err = np.abs(_np(out)[..., :128].astype(np.float64) - mo.conv1d(xd, wd).numpy())
    rel = (err / np.maximum(mo.conv1d(xd.abs(), wd.abs()).numpy(), 1e-30)).max()
    print('\none tap (two MFMAs): max err / sum|a w| = 2^%.1f' % np.log2(rel))
    assert 2.0 ** -21 < rel <= 2.0 ** -15, np.log2(rel)


BANK_SHAPES = [(2, 128), (8, 128), (32, 128), (16, 256), (32, 256)]


@pytest.mark.parametrize('K,Cin', BANK_SHAPES)
def test_bank_kernel_vs_float64_of_device_operands(K, Cin):
    """M = 1200 (3 windows of 400: not a multiple of the 127-frame tile step; SAME padding at both window edges)."""
    y32, _, ref, tol = _bank_case(K, Cin)
    err = np.abs(_np(y32).astype(np.float64) - ref)
    print('\nbank K=%d Cin=%d: max err %.2e, max err / tol %.3f' % (K, Cin, err.max(), (err / tol.clip(1e-30)).max()))
    assert np.all(err <= tol), (err.max(), np.unravel_index(np.argmax(err - tol), err.shape))


@pytest.mark.parametrize('K,Cin', [(32, 128), (16, 256), (32, 256)])
def test_bank_mx_epilogue_vs_cpu_quantiser_on_float64(K, Cin):
    """The device's fp8 codes and scales against tests/mx8_ref.quantize of the ORACLE's float64 values (not of the
    device's float32 ones).  Differences are allowed only where the float64 value lies within the kernel tolerance
    (module docstring) of a rounding midpoint -- the device's code is one RNE gives for a value within it -- or the
    block's amax within it of a scale boundary 448 * 2^e (one scale step); they are counted and must stay below 1e-3 of
    the elements."""
    _, ymx, ref, tol = _bank_case(K, Cin, seed=1)
    dc, ds = _np(ymx.codes).reshape(-1, 32), _np(ymx.scales).reshape(-1)
    rc, rs = mx.quantize(ref)
    rc, rs = rc.reshape(-1, 32), rs.reshape(-1)
    dc, rc = np.where(dc == 0x80, 0, dc), np.where(rc == 0x80, 0, rc)      # post-relu: -0 and +0 are the same zero
    ref_b, tol_b = ref.reshape(-1, 32), tol.reshape(-1, 32)
    n = ref.size
    exceptions = 0
    sbad = np.nonzero(ds != rs)[0]
    for b in sbad:
        amax, e = np.abs(ref_b[b]).max(), int(rs[b]) - 127
        assert abs(int(ds[b]) - int(rs[b])) == 1, (b, ds[b], rs[b])
        edge = 448.0 * 2.0 ** (e - 1 if ds[b] < rs[b] else e)
        assert abs(amax - edge) <= tol_b[b].max(), (b, amax, edge, tol_b[b].max())
        exceptions += 32
    same = ds == rs
    cbad = np.argwhere((dc != rc) & same[:, None])
    multi = 0
    for b, i in cbad:
        # the device's code must be one that RNE gives for SOME value within the tolerance of the float64 value
        # (post-relu values are >= 0): ref +- tol may straddle one midpoint -- or several, for a small element of its
        # block whose value came out of cancellation (|value| << sum |a w|)
        inv = 2.0 ** (127 - int(rs[b]))
        lo = mx.encode_scaled(np.array([max(ref_b[b, i] - tol_b[b, i], 0.0) * inv]))[0]
        hi = mx.encode_scaled(np.array([(ref_b[b, i] + tol_b[b, i]) * inv]))[0]
        assert lo <= dc[b, i] <= hi, (b, i, dc[b, i], rc[b, i], ref_b[b, i], tol_b[b, i], lo, hi)
        multi += abs(int(dc[b, i]) - int(rc[b, i])) > 1
        exceptions += 1
    # elements whose tolerance interval holds more than one RNE result: where a difference is possible at all
    inv = np.ldexp(1.0, 127 - rs.astype(np.int64))[:, None]
    amb = (mx.encode_scaled(np.maximum(ref_b - tol_b, 0) * inv) != mx.encode_scaled((ref_b + tol_b) * inv)) & same[:, None]
    print('\nbank K=%d Cin=%d MX epilogue: %d scale and %d code exceptions (%d of them more than one code step) in %d '
          'elements; %d elements lie within tolerance of a rounding midpoint' % (K, Cin, len(sbad), len(cbad), multi, n,
                                                                                 int(amb.sum())))
    # 1e-3, not the 1e-4 of a float32-accurate accumulation: the scaled MFMA sums to ~17 bits (module docstring), and
    # the share of values that close to a midpoint scales with that error (measured 3.7e-4)
    assert exceptions <= 1e-3 * n


# ------------------------------------------------------------------------------------------- 5. projection
@pytest.mark.parametrize('filters', [128, 256])
def test_projection_vs_float64_of_device_operands(filters):
    """conv1d_1's form: 4,096 MX channels (pooled bank output), width 3, 128 / 256 outputs, BN + relu, bf16 out; the
    float32 form of the same launch is checked against float64, and the bf16 output equals its RNE rounding."""
    import mx8
    import _vc
    rng = np.random.RandomState(7)
    N, T, Cin = 3, 400, 4096
    a = torch.from_numpy(np.maximum(rng.standard_normal((N * T, Cin)), 0).astype(np.float32)).cuda()
    xq, xs = mx8.quantize(a, N * T, Cin)
    X = mx8.MxTensor(xq.view(N, T, Cin), xs.view(N, T, Cin // 32))
    kern = torch.from_numpy(rng.uniform(-0.02, 0.02, (3, Cin, filters)).astype(np.float32)).cuda()
    w, ws = mx8.pack_kernel(kern)
    s = torch.from_numpy(rng.uniform(0.5, 2.0, filters).astype(np.float32)).cuda()
    sh = torch.from_numpy(rng.uniform(-0.3, 0.3, filters).astype(np.float32)).cuda()
    y32 = mx8.conv(X, (w, ws), 3, filters, s, sh, _vc.ACT_RELU, out_mode=_vc.MX8_OUT_F32)
    y16 = mx8.conv(X, (w, ws), 3, filters, s, sh, _vc.ACT_RELU)
    xd = torch.from_numpy(mx.dequantize(_np(xq), _np(xs)).reshape(N, T, Cin))
    wd = torch.from_numpy(mx.dequantize(_np(w), _np(ws)).T.reshape(3, Cin, filters).copy())
    sd, shd = torch.from_numpy(_np(s)).double(), torch.from_numpy(_np(sh)).double()
    ref = torch.relu(mo.conv1d(xd, wd) * sd + shd).numpy()
    tol = (mo.conv1d(xd.abs(), wd.abs()) * sd.abs() * _acc_tol(3 * Cin // 64) + shd.abs() * 2.0 ** -23).numpy()
    err = np.abs(_np(y32).astype(np.float64) - ref)
    print('\nprojection %d: max err %.2e, max err / tol %.3f' % (filters, err.max(), (err / tol.clip(1e-30)).max()))
    assert np.all(err <= tol)
    assert torch.equal(y16, y32.bfloat16())


# --------------------------------------------------------------------------------------- 6.-8. the decoder
def _dec_cfg(dtype):
    cfg = json.load(open(os.path.join(HP, 'decoder_cfg_d.json')))
    cfg.update(is_training=False, compute_dtype=dtype)
    return cfg


def _decoder(dtype, wd):
    import contextlib
    import io
    from decoder import decoder_specs
    with contextlib.redirect_stdout(io.StringIO()):
        dec = decoder_specs(_dec_cfg(dtype), None, None)
    dec.store.load_dict(dict(wd), strict=False)
    return dec


def _ppg(W, seed):
    rng = np.random.RandomState(seed)
    return torch.softmax(torch.from_numpy(rng.standard_normal((W, 400, 61)) * 3.0), -1).float().numpy()


def _oracle(ppg_sub, wd, cfg):
    # the decoder converts its input to bf16 first: the oracle sees the same posteriors
    p = torch.from_numpy(ppg_sub).bfloat16().double()
    with torch.no_grad():
        ym, ys = mo.decoder_forward(p, mo.to_torch(wd, torch.float64), cfg)
    return ym.numpy(), ys.numpy()


def _stats(a, b):
    d = np.abs(a - b)
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


@pytest.fixture(scope='module')
def weights():
    return mo.init_weights(_dec_cfg('float32'), 'decoder', seed=2, perturb_bn=True)


@pytest.mark.parametrize('W', [64, 128])
def test_mxfp8_decoder_at_bench_batch_vs_oracle(weights, W):
    dec = _decoder('mxfp8', weights)
    ref16 = _decoder('bfloat16', weights)
    x = _ppg(W, 20 + W)
    r = dec.predict(x, batch_size=W)
    assert any(k[0] == 'mx8bank' for k in dec.store._cache) and any(k[0] == 'mx8conv' for k in dec.store._cache)
    # the MX path builds no bf16 layout copies of the bank kernels
    assert not any(k[0] == 'conv' and '/conv1d_banks/' in k[1] for k in dec.store._cache if isinstance(k, tuple))
    r16 = ref16.predict(x, batch_size=W)
    assert r.y_mel.shape == (W, 400, 80) and r.y_stft.shape == (W, 400, 201) and r.y_mel.dtype == np.float32
    sub = [0, W // 2, W - 1]
    ym, ys = _oracle(x[sub], weights, _dec_cfg('float32'))
    for name, got, g16, ref in (('y_mel', r.y_mel[sub], r16.y_mel[sub], ym), ('y_stft', r.y_stft[sub], r16.y_stft[sub], ys)):
        s, s16 = _stats(got, ref), _stats(g16, ref)
        print('\nW=%d %s vs float64 oracle: mxfp8 max %.2e rms %.2e | bf16 max %.2e rms %.2e' % (W, name, s[0], s[1], s16[0], s16[1]))
        assert s[0] <= DER_MAX and s[1] <= DER_RMS, (name, s)          # (D)
        assert s[0] <= REG_MAX and s[1] <= REG_RMS, (name, s)          # (R)


def test_bf16_decoder_unchanged_by_an_mxfp8_decoder_in_the_same_process(weights):
    x = _ppg(4, 3)
    b = _decoder('bfloat16', weights)
    before = b.predict(x)
    m = _decoder('mxfp8', weights)
    rm = m.predict(x)
    after = b.predict(x)
    again = _decoder('bfloat16', weights).predict(x)
    for f in ('y_mel', 'y_stft'):
        assert np.array_equal(getattr(before, f), getattr(after, f)) and np.array_equal(getattr(before, f), getattr(again, f))
        assert not np.array_equal(getattr(before, f), getattr(rm, f))          # the mxfp8 decoder did run its own path


def test_public_api_predict_forward_and_weight_refresh(weights):
    x = _ppg(4, 9)
    dec = _decoder('mxfp8', weights)
    r = dec.predict(x)
    assert type(r).__name__ == 'predict' and r._fields == ('y_mel', 'y_stft', 'y_phn')
    assert r.y_mel.dtype == np.float32 and r.y_stft.dtype == np.float32 and r.y_mel.shape == (4, 400, 80)
    assert r.y_stft.shape == (4, 400, 201) and r.y_phn.shape == (4, 400, 61)
    f = dec.forward(torch.from_numpy(x).cuda())
    assert np.array_equal(_np(f['y_mel']), r.y_mel) and np.array_equal(_np(f['y_stft']), r.y_stft)
    # new weights through store.assign: the MX layout copies follow
    w2 = dict(weights)
    rng = np.random.RandomState(4)
    for k in list(w2):
        if '/conv1d_banks/' in k and k.endswith('/kernel') or '/conv1d_1/conv1d/kernel' in k:
            w2[k] = (w2[k] * rng.uniform(0.5, 1.5, w2[k].shape)).astype(np.float32)
            dec.store.assign(k, w2[k])
    r2 = dec.predict(x)
    assert not np.array_equal(r2.y_stft, r.y_stft)
    ym, ys = _oracle(x[:2], w2, _dec_cfg('float32'))
    for got, ref in ((r2.y_mel[:2], ym), (r2.y_stft[:2], ys)):
        s = _stats(got, ref)
        assert s[0] <= DER_MAX and s[1] <= DER_RMS, s


def test_encoder_with_mxfp8_raises():
    from encoder import encoder_spec_phn
    cfg = json.load(open(os.path.join(HP, 'encoder_cfg_d.json')))
    cfg.update(is_training=False, compute_dtype='mxfp8')
    with pytest.raises(ValueError, match='covers the decoder only'):
        encoder_spec_phn(cfg, None)
