"""Shapes and inputs of the spectral-mapping tests, shared by tests/test_mapping_cpu.py (which checks the float32 control
against every derived bound on exactly these inputs) and tests/test_mapping_gpu.py."""
import numpy as np

import mapping_ref as mr

TILE = 32                                               # vc_jd_tile(): cells / frames per tile
SOLVE_FRAMES = (1, 2, 3, 4, 5, 9, 46)                   # dense-solve check of the restatement
MLPG_LENS = [0, 1, 2, 3, 4, 5, 9, 46]                   # one ragged batch: every clamp pattern of the window, and a long one
MLPG_COEF = (1, 24, 32)
JD_SHAPES = [(1, 2), (2, 48), (63, 64), (64, 2), (65, 48), (256, 64)]       # (M, D)
MAP_LENS = [0, 1, 2, 3, 4, 5, 9, TILE - 1, TILE, TILE + 1]
SPREAD = 0.25                                           # of the components' means, in standard deviations: posteriors stay soft,
                                                        # so every component's sums come from cells it has a real share in (the
                                                        # 2 delta rule is derived for those; mapping_ref's docstring)
PAD = 3                                                 # rows behind the longest utterance
ACC_LENS_A = [70, 0, 33]                                # a ragged batch of 3 with a zero-length utterance
ACC_LENS_B = [50, 40, 33]
GAIN_CASES = [(1, 3), (24, 9), (32, 5)]                 # (n_coef, frames)


def mlpg_case(n, lens=MLPG_LENS, seed=0):
    """P [B, maxF, 2 n] in [0.5, 5), R = P * E with E of order 1; rows at or beyond a length are NaN (never read)."""
    rng = np.random.RandomState(100 + seed + n)
    B, F = len(lens), max(lens) + PAD
    P = rng.uniform(0.5, 5.0, (B, F, 2 * n)).astype(np.float32)
    R = (P * rng.standard_normal((B, F, 2 * n))).astype(np.float32)
    for b, l in enumerate(lens):
        P[b, l:], R[b, l:] = np.nan, np.nan
    return P, R


def draw(model, n, rng):
    """n joint vectors near the model's components."""
    M, D = model['mu_x'].shape
    m = rng.randint(0, M, n)
    x = model['mu_x'][m] + np.sqrt(model['var_x'][m]) * rng.standard_normal((n, D))
    y = model['mu_y'][m] + np.sqrt(model['var_y'][m]) * rng.standard_normal((n, D))
    return x.astype(np.float32), y.astype(np.float32)


def monotone_path(la, lb, rng):
    i = j = 0
    out = [(0, 0)]
    while i < la - 1 or j < lb - 1:
        step = rng.randint(0, 3)
        if i == la - 1:
            step = 2
        elif j == lb - 1:
            step = 1
        i, j = i + (step != 2), j + (step != 1)
        out.append((i, j))
    return out


def acc_case(M, D, with_path=True, seed=0):
    """(model, feat_a [3, Fa, D], feat_b [3, Fb, D], lens_a, lens_b, path [3, max_path, 2] | None, path_len | None): the path
    holds (-1, -1) cells, cells beyond the lengths and junk behind path_len; feature rows beyond a length are NaN."""
    rng = np.random.RandomState(200 + seed + 7 * M + D)
    model = mr.random_model(M, D, seed=seed + M + D, spread=SPREAD)
    Fa, Fb = max(ACC_LENS_A) + PAD, max(ACC_LENS_B) + PAD
    fa, fb = np.full((3, Fa, D), np.nan, np.float32), np.full((3, Fb, D), np.nan, np.float32)
    for b in range(3):
        x, y = draw(model, max(ACC_LENS_A[b], ACC_LENS_B[b]), rng)
        fa[b, :ACC_LENS_A[b]], fb[b, :ACC_LENS_B[b]] = x[:ACC_LENS_A[b]], y[:ACC_LENS_B[b]]
    if not with_path:
        return model, fa, fb, ACC_LENS_A, ACC_LENS_B, None, None
    max_path = Fa + Fb - 1
    path = np.full((3, max_path, 2), 0x7FFFFFFF, np.int32)
    plen = np.zeros(3, np.int32)
    for b in range(3):
        la, lb = ACC_LENS_A[b], ACC_LENS_B[b]
        cells = monotone_path(la, lb, rng) if la and lb else [(0, 0), (1, 1)]
        cells = cells[:5] + [(-1, -1)] + cells[5:] + [(la, 0), (0, lb), (-1, -1), (la + 5, lb + 5)]
        path[b, :len(cells)] = cells
        plen[b] = len(cells)
    plen[2] = max_path + 50                              # clamped to max_path; the junk behind the cells is out of range
    path[2, len(cells):] = -1
    return model, fa, fb, ACC_LENS_A, ACC_LENS_B, path, plen


def map_case(M, D, seed=1):
    """(model, feat [B, F, D] with NaN rows beyond the lengths, lens).  Seed 1: no frame's two largest l_m lie within 2 delta
    (seed 0 has one such frame at M = 63; tests/test_mapping_cpu.py asserts the margin)."""
    rng = np.random.RandomState(300 + seed + 5 * M + D)
    model = mr.random_model(M, D, seed=seed + M + D, spread=SPREAD)
    B, F = len(MAP_LENS), max(MAP_LENS) + PAD
    feat = np.full((B, F, D), np.nan, np.float32)
    for b, l in enumerate(MAP_LENS):
        feat[b, :l] = draw(model, l, rng)[0]
    return model, feat, MAP_LENS


def gain_case(n, F, n_mels=80, seed=0):
    rng = np.random.RandomState(400 + seed + n)
    cy = (0.05 * rng.standard_normal((3, F + PAD, n))).astype(np.float32)
    cx = (0.05 * rng.standard_normal((3, F + PAD, n))).astype(np.float32)
    nf = [F, 0, max(F - 2, 0)]
    for b in range(3):
        cy[b, nf[b]:], cx[b, nf[b]:] = np.nan, np.nan
    return cy, cx, nf


CFG = dict(sample_rate=16000, pre_emphasis=0.97, hop_length=80, win_length=400, n_mels=80, n_mfcc=40, n_fft=None, window='hann',
           mfcc_normaleze_first_mfcc=True, mfcc_norm_factor=0.01, calc_mfcc_derivate=True, M_dB_norm_factor=0.01,
           P_dB_norm_factor=0.01, mean_abs_amp_norm=0.003, clip_output=True)
