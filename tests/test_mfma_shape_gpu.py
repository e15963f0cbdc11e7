"""The fragment and accumulator maps of v_mfma_f32_16x16x32_bf16 in bank256_kernel (filter bank and wide projection) and
conv256_kernel, at the places the shapes of tests/test_conv_gemm_gpu.py do not reach: every tap offset of the LDS swizzle,
a window edge inside a 16-frame tile, two slabs, the K split at its least size, a one-hot input whose every output
element names the fragment slot it came from, and conv256's operand pool with signed zeros.  Integer-grid operands
(tests/mfma_shape_cases.py; proven exact in tests/test_mfma_shape_cpu.py): the device must EQUAL the float64 reference,
twice with identical bits, and identically with the kernel's option switched off."""
import numpy as np
import pytest
import torch

import conv_gemm_ref as R
from conv_gemm_cases import expected_form, make_exact
from mfma_shape_cases import BANK_CIN128, BANK_TAPS, CONV256, ONE_HOT, ONE_HOT_AT, PROJ_SPLIT, make_one_hot, signed_zero_pool
from test_conv_gemm_gpu import Launch, _host, _run_exact, _run_twice, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_kernel_options():
    import _vc
    yield
    for n in ('bank256', 'conv256', 'proj256', 'proj256_split'):
        _vc.set_option(n, -1)


def test_bank_every_tap_residue():
    """Widths 1..32 on two windows of 130 frames: taps 0..31, a window edge inside a fragment tile, clamped rows past M."""
    assert expected_form(BANK_TAPS) == 'bank256'
    _run_exact(BANK_TAPS)


@pytest.mark.parametrize('s', BANK_CIN128, ids=[s.name for s in BANK_CIN128])
def test_bank_two_slabs(s):
    assert expected_form(s) == 'bank256'
    _run_exact(s)


@pytest.mark.parametrize('frame,ch', ONE_HOT_AT)
def test_bank_one_hot_placement(frame, ch):
    """One 1.0 at (frame, ch); the weights encode (filter, output channel, tap, channel): an element taken from another
    fragment slot, or put into another accumulator position, shows as a wrong integer or a non-zero where zero belongs."""
    assert expected_form(ONE_HOT) == 'bank256'
    d = make_one_hot(frame, ch)
    ref = R.conv_gemm(d)
    what = 'one-hot at frame %d channel %d' % (frame, ch)
    _same(_host(_run_twice(Launch(d, ONE_HOT.ldx), what)), ref, what)


@pytest.mark.parametrize('s', PROJ_SPLIT, ids=[s.name for s in PROJ_SPLIT])
def test_projection_split_equals_unsplit(s):
    """K split over two workgroups (the slab exchange stores and adds the accumulators in register order): exact, and bit for
    bit what the unsplit launch and conv256_kernel give (the toggles of the case)."""
    import ctypes as C
    import _vc
    assert expected_form(s) == 'proj256'
    L, _, _ = _run_exact(s)
    assert L.desc.d_workspace and _vc.lib().vc_conv_gemm_workspace_bytes(C.byref(L.desc)) > 0


@pytest.mark.parametrize('s', CONV256, ids=[s.name for s in CONV256])
def test_conv256(s):
    assert expected_form(s) == 'conv256'
    _run_exact(s)
    if s.pro_pool == 2:
        # -0.0 next to a positive value, and as the window's last frame, through the maximum taken on the fragments
        d = signed_zero_pool(s, make_exact(s))
        L = Launch(d, s.ldx)
        assert bool(torch.signbit(L.X[:, :s.Cin].float()).any())
        _same(_host(_run_twice(L, s.name + ' signed zeros')), R.conv_gemm(d), s.name + ' signed zeros')
