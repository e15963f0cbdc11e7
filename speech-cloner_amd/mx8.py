"""MX-FP8 inference of the decoder's filter banks and the projection behind them (include/vc_hip.h "MX-FP8",
csrc/vc_mx8.hip).  Opt-in: ``VariableStore(compute_dtype='mxfp8')`` runs everything in bf16 except, per CBHG,

  conv1d_banks + max_pooling1d (the reference's modules.py:144-166, 331)  -> vc_mx8_conv, MX-FP8 output
  conv1d_1 (the reference's modules.py:333-335) on that MX-FP8 tensor      -> vc_mx8_conv, bf16 output

Format: OCP MX-FP8 (e4m3fn elements, one E8M0 scale per 32 channels); weights are quantised once per weight version
from the float32 masters, transposed to [Cout, taps * Cin] like the bf16 layout, and cached under their own keys
(('mx8bank', scope), ('mx8conv', scope, bn_scope)), so ``store.invalidate()`` drops them with every other layout copy.

Shapes the MX kernel covers (else the bf16 kernels run): the bank needs an even number of widths K <= 32, 128 filters
per width and a channel count that is a multiple of 64 (the decoder's 128 / 256; not the encoder's 40, nor the small
test configurations); conv1d_1 needs a multiple of 128 output channels (embed_size // 2 = 128 / 256).
"""
import ctypes as C

import _vc

BANK_FILTERS = 128


def _torch():
    import torch
    return torch


class MxTensor:
    """An MX-FP8 activation [N, T, C]: ``codes`` uint8 e4m3fn [N, T, C], ``scales`` uint8 E8M0 [N, T, C // 32]."""

    def __init__(self, codes, scales):
        self.codes, self.scales = codes, scales

    @property
    def shape(self):
        return self.codes.shape


def bank_supported(K, Cin, F_):
    return K % 2 == 0 and 2 <= K <= 32 and F_ == BANK_FILTERS and Cin % 64 == 0


def conv_supported(Cin, filters, size):
    return Cin % 64 == 0 and filters % 128 == 0 and filters // 128 <= _vc.MX8_MAX_GROUPS and 1 <= size <= 32


def quantize(x2d, M, Cn, ldx=None):
    """bf16 / float32 [M, >= Cn] (row stride ldx) -> (codes uint8 [M, Cn], scales uint8 [M, Cn // 32])."""
    torch = _torch()
    codes = torch.empty((M, Cn), dtype=torch.uint8, device=x2d.device)
    scales = torch.empty((M, Cn // 32), dtype=torch.uint8, device=x2d.device)
    dt = {torch.float32: _vc.VC_F32, torch.bfloat16: _vc.VC_BF16}[x2d.dtype]
    _vc.check(_vc.lib().vc_mx8_quantize(x2d.data_ptr(), dt, M, Cn, Cn if ldx is None else ldx, codes.data_ptr(),
                                        scales.data_ptr(), _vc.current_stream()))
    return codes, scales


def pack_kernel(kernel):
    """TF-layout float32 kernel [k, Cin, Cout] -> MX weights of W^T [Cout, k * Cin] (blocks = (output channel, tap, 32
    input channels))."""
    k, cin, cout = kernel.shape
    wt = kernel.reshape(k * cin, cout).t().contiguous().float()
    return quantize(wt, cout, k * cin)


def _launch(X, Xs, M, T, Cin, groups, scale, shift, act, pool, out_mode, n_out, out, out_s=None):
    torch = _torch()
    lib = _vc.lib()
    d = _vc.Mx8ConvDesc()
    d.d_X, d.d_Xs, d.M, d.T, d.Cin, d.n_groups = X.data_ptr(), Xs.data_ptr(), M, T, Cin, len(groups)
    for i, (w, ws, taps, pad_l, c_off) in enumerate(groups):
        g = d.groups[i]
        g.d_W, g.d_Ws, g.taps, g.pad_l, g.c_off = w.data_ptr(), ws.data_ptr(), taps, pad_l, c_off
    d.d_epi_scale, d.d_epi_shift = scale.data_ptr(), shift.data_ptr()
    d.act, d.pool, d.out_mode, d.n_out = act, int(pool), out_mode, n_out
    d.d_C, d.d_Cs = out.data_ptr(), (out_s.data_ptr() if out_s is not None else None)
    nbytes = lib.vc_mx8_conv_workspace_bytes(C.byref(d))
    if nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
        d.d_workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    _vc.check(lib.vc_mx8_conv(C.byref(d), _vc.current_stream()))


def bank_groups(packed, K, Cin):
    """Launch groups of the packed bank: width k = 1..K, SAME left padding (k - 1) // 2, output channels 128 (k - 1)."""
    return [(w, ws, k, (k - 1) // 2, BANK_FILTERS * (k - 1)) for k, (w, ws) in zip(range(1, K + 1), packed)]


def bank(x, packed, K, scale, shift, out_mode=_vc.MX8_OUT_MX):
    """Filter bank + folded BN + relu + max_pool(2, 1, same) of x [N, T, Cin] (bf16): -> MxTensor [N, T, 128 K]
    (out_mode MX) or a float32 / bf16 tensor (tests)."""
    torch = _torch()
    N_, T_, Cin = x.shape
    M = N_ * T_
    xq, xs = quantize(x.contiguous().view(M, Cin), M, Cin)
    n_out = BANK_FILTERS * K
    if out_mode == _vc.MX8_OUT_MX:
        out = torch.empty((N_, T_, n_out), dtype=torch.uint8, device=x.device)
        out_s = torch.empty((N_, T_, n_out // 32), dtype=torch.uint8, device=x.device)
    else:
        out = torch.empty((N_, T_, n_out), dtype=torch.float32 if out_mode == _vc.MX8_OUT_F32 else torch.bfloat16,
                          device=x.device)
        out_s = None
    _launch(xq, xs, M, T_, Cin, bank_groups(packed, K, Cin), scale, shift, _vc.ACT_RELU, 1, out_mode, n_out, out, out_s)
    return MxTensor(out, out_s) if out_mode == _vc.MX8_OUT_MX else out


def conv(mx, packed, size, filters, scale, shift, act, out_mode=_vc.MX8_OUT_BF16):
    """SAME convolution of an MxTensor [N, T, Cin] with the packed kernel (pack_kernel) + folded BN + act -> bf16
    (or float32 with out_mode F32) [N, T, filters]."""
    torch = _torch()
    w, ws = packed
    N_, T_, Cin = mx.shape
    M = N_ * T_
    Kw = size * Cin
    groups = [(w[g * 128:(g + 1) * 128], ws[g * 128:(g + 1) * 128], size, (size - 1) // 2, g * 128)
              for g in range(filters // 128)]
    out = torch.empty((N_, T_, filters), dtype=torch.float32 if out_mode == _vc.MX8_OUT_F32 else torch.bfloat16,
                      device=mx.codes.device)
    assert w.shape == (filters, Kw)
    _launch(mx.codes, mx.scales, M, T_, Cin, groups, scale, shift, act, 0, out_mode, filters, out)
    return out
