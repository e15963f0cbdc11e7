"""CPU reference of the MX-FP8 format (include/vc_hip.h "MX-FP8") and a float64 decoder forward that simulates it.

Written independently of the device quantiser (csrc/vc_mx8.h, integer bit manipulation): here the e4m3fn code table
is spelled out value by value, the scale exponent comes from numpy's frexp, and rounding is a nearest-neighbour search
in the table with ties to the even code.

Format: a block is 32 consecutive elements along the last axis.  Scale rule: e is the smallest integer with
amax <= 448 * 2^e, clamped to [-127, 127], E8M0 code e + 127.  Elements: RNE(x * 2^-e) in e4m3fn, subnormals kept,
sign bit = sign of x.  An all-zero block: scale code 0, elements 0x00.

Not a test module (no test_ prefix): tests/test_mx8_cpu.py and tests/test_mx8_gpu.py import it.
"""
import numpy as np
import torch

from oracle import model_oracle as mo


def _e4m3fn_table():
    t = np.zeros(256, dtype=np.float64)
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan                                   # 0x7F / 0xFF: the only NaNs; e4m3fn has no infinities
        elif e == 0:
            v = (m / 8.0) * 2.0 ** -6                    # subnormals m * 2^-9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if s else v
    return t


E4M3 = _e4m3fn_table()
POS = E4M3[:127]                # codes 0x00 .. 0x7E: 0 .. 448, increasing
MAX = 448.0


def scale_exp(amax):
    """e of the block scale for amax > 0 (array)."""
    fr, ex = np.frexp(np.asarray(amax, dtype=np.float64))        # amax = fr 2^ex, fr in [0.5, 1) = (f / 2) 2^(ea + 1)
    e = np.where(fr <= 0.875, ex - 9, ex - 8)                     # f = 2 fr <= 1.75: e = ea - 8, else ea - 7
    return np.clip(e, -127, 127).astype(np.int64)


def encode_scaled(v):
    """|v| <= 448 (float64 array) -> e4m3fn code of RNE(|v|) without sign."""
    a = np.abs(v)
    hi = np.clip(np.searchsorted(POS, a, side='left'), 0, 126)   # first code >= a
    lo = np.clip(hi - 1, 0, 126)
    dlo, dhi = a - POS[lo], POS[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    return np.where(a == POS[hi], hi, np.where(pick_hi, hi, lo)).astype(np.uint8)


def quantize(x):
    """x [..., C] (float32 values, any float dtype), C % 32 == 0 -> (codes uint8 [..., C], scales uint8 [..., C/32])."""
    x = np.asarray(x, dtype=np.float64)
    sh = x.shape
    xb = x.reshape(sh[:-1] + (sh[-1] // 32, 32))
    amax = np.abs(xb).max(-1)
    nz = amax > 0
    e = np.where(nz, scale_exp(np.where(nz, amax, 1.0)), 0)
    v = np.abs(xb) * np.ldexp(1.0, -e)[..., None]
    assert np.all(v <= MAX)
    codes = encode_scaled(v) | (np.signbit(xb).astype(np.uint8) << 7)
    codes = np.where(nz[..., None], codes, 0).astype(np.uint8)
    scales = np.where(nz, e + 127, 0).astype(np.uint8)
    return codes.reshape(sh), scales


def dequantize(codes, scales):
    codes = np.asarray(codes)
    v = E4M3[codes.astype(np.int64)]
    s = np.ldexp(1.0, np.asarray(scales, dtype=np.int64) - 127)
    return (v.reshape(codes.shape[:-1] + (-1, 32)) * s[..., None]).reshape(codes.shape)


def qdq(x):
    """Quantise then dequantise along the last axis (numpy float64 in/out)."""
    return dequantize(*quantize(x))


def qdq_t(x):
    """qdq of a torch tensor, float64 result on the same device."""
    return torch.from_numpy(qdq(x.detach().cpu().numpy())).to(x.device, torch.float64)


def qdq_kernel(k):
    """TF-layout kernel [taps, Cin, Cout]: blocks = (output channel, tap, 32 input channels), as the device packs it."""
    taps, cin, cout = k.shape
    wt = k.detach().cpu().numpy().astype(np.float64).reshape(taps * cin, cout).T       # [Cout, taps * Cin]
    return torch.from_numpy(qdq(wt).T.reshape(taps, cin, cout).copy()).to(k.device, torch.float64)


# --------------------------------------------------------------------- where the device runs MX (speech-cloner_amd/mx8.py)
def bank_supported(K, Cin, F_=128):
    return K % 2 == 0 and 2 <= K <= 32 and F_ == 128 and Cin % 64 == 0


def cbhg_mx(x, w, scope, K, n_highway, proj_filters):
    """model_oracle.cbhg in float64 with the MX-FP8 roundings of the device: the bank's input and weights, its pooled
    output (the projection's input) and the projection's weights.  Shapes the device keeps on bf16 are not rounded."""
    if not (bank_supported(K, x.shape[-1]) and proj_filters % 128 == 0):
        return mo.cbhg(x, w, scope, K, n_highway)
    bs = scope + '/conv1d_banks'
    xq = qdq_t(x)
    outs = [mo.conv1d(xq, qdq_kernel(w[bs + ('/conv1d' if k == 1 else '/num_%d/conv1d' % k) + '/conv1d/kernel']))
            for k in range(1, K + 1)]
    y = torch.relu(mo.bn(torch.cat(outs, dim=-1), w, bs + '/bn'))
    y = qdq_t(mo.max_pool_2_same(y))
    y = mo.conv1d(y, qdq_kernel(w[scope + '/conv1d_1/conv1d/kernel']))
    y = torch.relu(mo.bn(y, w, scope + '/conv1d_1'))
    y = mo.bn(mo.conv1d(y, w[scope + '/conv1d_2/conv1d/kernel']), w, scope + '/conv1d_2') + x
    for i in range(n_highway):
        y = mo.highwaynet(y, w, scope + '/highwaynet_%d' % i)
    return mo.gru_bidirectional(y, w, scope + '/gru')


def decoder_forward_mx(ppg, w, cfg):
    """model_oracle.decoder_forward (inference, use_target_mel_step2 false) with cbhg_mx.  -> (y_mel, y_stft)."""
    scope = cfg.get('model_name', 'decoder')
    x = ppg
    ys = []
    for i, sd in enumerate(cfg['steps_v']):
        s = '%s/step%d' % (scope, i + 1)
        pre = mo.prenet(x, w, s + '/prenet', cfg['dropout_rate'])
        E = pre.shape[-1] * 2
        out = cbhg_mx(pre, w, s + '/CBHG', sd['num_conv_banks'], sd['num_highwaynet_blocks'], E // 2)
        x = mo.dense(out, w, s + '/y_logits')
        ys.append(x)
    return ys[0], ys[1]
