"""Soundness of tests/mfma_shape_cases.py without a GPU: every case takes the kernel form it is meant for, and stays on the
integer grid on which float32 sums are exact in any order and every bf16 result is an integer of magnitude <= 256."""
import numpy as np
import pytest

import conv_gemm_ref as R
from conv_gemm_cases import exactness, expected_form, make_exact
from mfma_shape_cases import CONV256, EXACT, ONE_HOT, ONE_HOT_AT, make_one_hot, signed_zero_pool, weight_code


def _sound(s, d):
    big, stored, grid = exactness(s, d)
    assert big < 2.0 ** 24 and grid and stored <= 256.0, (s.name, big, stored, grid)
    assert all(np.array_equal(R.bf16_round(g.W), g.W) for g in d.groups) and np.array_equal(R.bf16_round(d.X), d.X)


@pytest.mark.parametrize('s', EXACT, ids=[s.name for s in EXACT])
def test_cases_take_their_form_and_stay_exact(s):
    assert expected_form(s) == s.form
    for opt in s.toggle:
        assert expected_form(s, {opt: 0}) != s.form or opt == 'proj256_split'
    _sound(s, make_exact(s))


def test_signed_zero_variant_of_the_pooled_operand():
    s = [c for c in CONV256 if c.pro_pool == 2][0]
    d = signed_zero_pool(s, make_exact(s))
    X = d.X.reshape(s.M // s.T, s.T, -1)
    assert np.signbit(X[:, 99]).all() and (np.signbit(X[:, 3]) & (X[:, 4] > 0)).any() and (d.X >= 0).all()
    _sound(s, d)


def test_one_hot_names_its_source():
    assert expected_form(ONE_HOT) == 'bank256'
    s = ONE_HOT
    for frame, ch in ONE_HOT_AT:
        d = make_one_hot(frame, ch)
        _sound(s, d)
        ref = R.conv_gemm(d)
        for g, taps in enumerate(s.taps):
            blk = ref[:, s.c_off[g]:s.c_off[g] + s.N]
            want = np.zeros_like(blk)
            for j in range(taps):
                m = frame - j + s.pad_l[g]
                if m // s.T == frame // s.T and 0 <= m < s.M:
                    want[m] = weight_code(g, np.arange(s.N), j, ch)
            assert np.array_equal(blk, want), (frame, ch, g)
