"""Shape tables and input builders of tests/test_score_kernels_{cpu,gpu}.py: the scoring launches of csrc/vc_dtw.hip,
csrc/vc_f0.hip and csrc/vc_activity.hip, each alone.  numpy only: tests/test_score_kernels_cpu.py proves every case usable
without a device (integer costs, every tile size reached, the reference's own marginal frames under the cap) and holds the
bounds; the references are tests/mcd_ref.py, tests/f0_ref.py and tests/activity_ref.py.

Every reference is computed once per process (functools.lru_cache) and never modified by a test."""
import functools
import math

import numpy as np

import f0_ref as fr
import mcd_ref as mr

EPS = 2.0 ** -24                      # the unit round-off of float32
LDS_BUDGET = 64 * 1024

# ---------------------------------------------------------------------------------------------------- DTW
# (n_coef, [(Fa, Fb), ...]): one ragged batch per n_coef.  A pass is 1,024 rows (2049: three passes), the ring 512
# columns refilled every 256, sixteen codes to a word; n_coef on an instantiation's width (8, 16, 24, 32) and one past it.
DTW_EXACT = [
    (1, [(1, 1), (5, 257), (1024, 512)]),
    (8, [(1, 15), (1025, 513)]),
    (9, [(3, 1), (1023, 511), (4, 16)]),
    (16, [(4, 256), (2049, 257)]),
    (17, [(5, 17), (1024, 512)]),
    (24, [(1023, 255), (3, 16)]),
    (25, [(1025, 1025), (1, 17)]),
    (32, [(2049, 257), (5, 255), (1024, 512)]),
]
DTW_PAD_A, DTW_PAD_B = 3, 5           # max_a = longest Fa + 3, max_b = longest Fb + 5: NaN rows behind every utterance
DTW_BAND = [(8, (1025, 513)), (9, (5, 17)), (32, (4, 16)), (17, (257, 255))]
DTW_REAL = [(24, (257, 300)), (17, (1025, 513))]
REAL_SCALE = 25.0


def int_cepstra(rng, F, n_coef, hi=4):
    """Frames whose distances are integers: an integer k per frame in every column when 2 n_coef is a square (d = sqrt(2
    n_coef) |dk|), else in the first and the last column only (d = 2 |dk|), the columns between holding the same
    non-zero constants on both sides.  n_coef = 1: d = sqrt(2) |dk| rounded, see dtw_exact_reference."""
    k = rng.randint(0, hi, (F, 1)).astype(np.float32)
    if n_coef == 1 or math.isqrt(2 * n_coef) ** 2 == 2 * n_coef:
        return k * np.ones((1, n_coef), np.float32)
    out = np.tile(np.arange(1, n_coef + 1, dtype=np.float32), (F, 1))
    out[:, 0] = k[:, 0]
    out[:, -1] = k[:, 0]
    return out


@functools.lru_cache(maxsize=None)
def dtw_exact_pairs(n_coef):
    pairs = dict(DTW_EXACT)[n_coef]
    rng = np.random.RandomState(100 + n_coef)
    return [(int_cepstra(rng, Fa, n_coef), int_cepstra(rng, Fb, n_coef)) for Fa, Fb in pairs]


def dtw_ref_dtype(n_coef):
    """float64 where every cost is an integer.  n_coef = 1 has d = scale * sqrt(2 dk^2), never an integer: there the
    reference is mcd_ref.dtw in float32, which is the same recurrence on the same correctly rounded d (one product, one
    correctly rounded square root, one product), so totals and paths are still equal exactly."""
    return np.float32 if n_coef == 1 else np.float64


@functools.lru_cache(maxsize=None)
def dtw_exact_reference(n_coef, k, band=None):
    a, b = dtw_exact_pairs(n_coef)[k]
    return mr.dtw(a, b, 1.0, band, dtw_ref_dtype(n_coef))


@functools.lru_cache(maxsize=None)
def dtw_band_pair(n_coef, Fa, Fb):
    rng = np.random.RandomState(7 * n_coef + Fa)
    a, b = int_cepstra(rng, Fa, n_coef), int_cepstra(rng, Fb, n_coef)
    free = mr.dtw(a, b, 1.0, None, dtw_ref_dtype(n_coef))
    p = free[2]
    v = int(np.abs(p[:, 1] * (Fa - 1) - p[:, 0] * (Fb - 1)).max())
    need = -(-v // max(Fa - 1, Fb - 1, 1))                             # the narrowest band that holds the free optimum
    return a, b, free, need


@functools.lru_cache(maxsize=None)
def dtw_band_reference(n_coef, Fa, Fb, band):
    a, b, _, _ = dtw_band_pair(n_coef, Fa, Fb)
    return mr.dtw(a, b, 1.0, band, dtw_ref_dtype(n_coef))


@functools.lru_cache(maxsize=None)
def dtw_real_pair(n_coef, Fa, Fb):
    """Smooth cepstra (a random walk per coefficient, the size of the front-end's), side b side a warped to Fb frames
    plus noise; float32 on both sides; the float64 optimum and the float32 restatement."""
    rng = np.random.RandomState(Fa + n_coef)
    a = np.cumsum(0.02 * rng.standard_normal((Fa, n_coef)), axis=0)
    pos = (Fa - 1) * np.linspace(0.0, 1.0, Fb) ** 1.3
    b = np.stack([np.interp(pos, np.arange(Fa), a[:, d]) for d in range(n_coef)], 1) + 0.01 * rng.standard_normal((Fb, n_coef))
    a, b = a.astype(np.float32), b.astype(np.float32)
    t64, n64, _ = mr.dtw(a, b, REAL_SCALE, None, np.float64, want_path=False)
    t32, n32, _ = mr.dtw(a, b, REAL_SCALE, None, np.float32, want_path=False)
    return a, b, float(t64), float(t32)


def dtw_real_bound(Fa, Fb, n_coef):
    """_check_real of tests/test_mcd_gpu.py, restated for any n_coef: a path has at most Fa + Fb - 1 cells, a distance
    n_coef + 2 roundings, so a total differs from its own path's float64 cost by at most (Fa + Fb + n_coef + 2) eps
    relative, and the device's path from the optimum by twice that."""
    return 2.0 * (Fa + Fb + n_coef + 2) * EPS


# ---------------------------------------------------------------------------------------------------- frame MCD, cepstra
FRAME_MCD_PAIRS = [(1, 4), (300, 255), (256, 256), (257, 700), (600, 513)]      # min: 1, 255, 256, 257, 513
FRAME_MCD_COEF = (1, 13, 33)
FRAME_PAD_A, FRAME_PAD_B = 2, 9


def frame_mcd_bound(n, n_coef):
    """Relative: a distance takes one subtraction, n_coef fused multiply-adds, the doubling (exact), a square root and a
    product: n_coef + 3 roundings on non-negative terms; a lane adds ceil(n / 256) of them, the tree eight levels, the
    division one more."""
    k = n_coef + 3 + -(-n // 256) + 8 + 1
    return k * EPS / (1.0 - k * EPS)


CEPSTRA_ROWS = (1, 255, 257)
CEPSTRA_SHAPES = ((1, 1), (80, 24), (512, 32))          # (n_mels, n_coef); 512 x 32 floats are exactly 64 KB of LDS
CEPSTRA_LONG = (32800, 40, 32)                          # rows * n_coef > 4,096 * 256: the grid-stride loop's second trip


def cepstra_bound(tab, mel):
    """Element by element: n_mels fused multiply-adds in one chain, gamma_n sum |t| |x| (the table is the float32 one on
    both sides, bf16 widens exactly)."""
    n = tab.shape[1]
    return (n * EPS / (1.0 - n * EPS)) * (np.abs(np.asarray(mel, np.float64)) @ np.abs(np.asarray(tab, np.float64)).T)


# ---------------------------------------------------------------------------------------------------- YIN
def yin_lanes(tau_max):
    return (tau_max + 2 + 63) & ~63


def yin_lds_bytes(W, tau_max, hop, G, cand=False):
    """csrc/vc_f0.hip, restated: the stage, one d' per lane, 64 words of the waves' totals (128 for the candidates)."""
    return (W + tau_max + 1 + (G - 1) * hop + yin_lanes(tau_max) + (128 if cand else 64)) * 4


def yin_tile(W, tau_max, hop, cand=False):
    G = 16
    while G > 1 and yin_lds_bytes(W, tau_max, hop, G, cand) > LDS_BUDGET:
        G >>= 1
    return G


SR = 16000.0
THRESHOLD = 0.15
# name: (W, hop, tau_min, tau_max)
YIN_CONFIGS = {
    'shipped': (512, 80, 40, 267),
    'one_wave': (96, 32, 8, 62),            # 64 lags: one wave, no idle lane
    'spill': (96, 32, 8, 63),               # 65 lags: 63 lanes of the second wave repeat the last lag
    'largest': (2048, 256, 100, 1022),      # 16 waves, the largest stage
    'w1': (1, 16, 8, 40),
    'w7': (7, 16, 8, 40),
    'w8': (8, 16, 8, 40),
    'w9': (9, 16, 8, 40),
    'one_lag': (64, 20, 30, 30),
    'tau_min_1': (64, 20, 1, 50),
    'g8': (64, 2000, 8, 62),
    'g4': (64, 4000, 8, 62),
    'g2': (64, 9000, 8, 62),
    'g1': (64, 17000, 8, 62),
}
YIN_TILES = {'g8': 8, 'g4': 4, 'g2': 2, 'g1': 1}      # every other configuration: 16
YIN_NCAND = {name: (1, 2, 15)[k % 3] for k, name in enumerate(YIN_CONFIGS)}


def yin_lengths(name):
    W, hop, _, tau_max = YIN_CONFIGS[name]
    G = yin_tile(W, tau_max, hop)
    long_row = 8000 if name == 'shipped' else G * hop + hop + 3          # 'shipped': a row of 101 frames for the 1 % cap
    return [0, 1, hop - 1, hop, G * hop - 1, G * hop, G * hop + 1, long_row]


def tone(name, n, phase=0.0):
    """A steady tone of a non-integer period inside the lag range with a second harmonic and a deterministic ripple:
    d' falls far below the threshold at the period and nowhere else near it."""
    W, hop, tau_min, tau_max = YIN_CONFIGS[name]
    P = tau_min + 0.2 if tau_min == tau_max else 0.5 * (tau_min + tau_max) + 0.37
    i = np.arange(n, dtype=np.float64)
    x = np.sin(2 * np.pi * i / P + phase) + 0.3 * np.sin(4 * np.pi * i / P + 1.0 + phase) + 1e-3 * np.sin(0.7391 * i * i)
    return (0.25 * x).astype(np.float32)


def yin_rows(name):
    lens = yin_lengths(name)
    base = tone(name, max(lens))
    return [base[:n] for n in lens]


@functools.lru_cache(maxsize=None)
def yin_reference(name):
    """Per row: (float64 (f0, ap, details), float32 restatement (f0, ap))."""
    W, hop, tau_min, tau_max = YIN_CONFIGS[name]
    kw = dict(sr=SR, hop=hop, W=W, threshold=THRESHOLD, tau_min=tau_min, tau_max=tau_max)
    return [(fr.yin(r, details=True, **kw), fr.yin(r, dtype=np.float32, **kw)) for r in yin_rows(name)]


@functools.lru_cache(maxsize=None)
def cand_reference(name, n_cand=None, ceiling=1.0):
    W, hop, tau_min, tau_max = YIN_CONFIGS[name]
    n_cand = n_cand or YIN_NCAND[name]
    return [(fr.candidates(r, SR, hop, W, tau_min, tau_max, n_cand, ceiling),
             fr.candidates(r, SR, hop, W, tau_min, tau_max, n_cand, ceiling, np.float32)) for r in yin_rows(name)]


NO_CAND_CEILING = 1e-7               # below every d' of the longest row of these configurations
NO_CAND_CONFIGS = ('shipped', 'w7', 'spill')

# many local minima: a short period in a wide lag range
MANY = dict(W=128, hop=64, tau_min=8, tau_max=200, period=10.3, n=2000)
MANY_KEEP = slice(3, 29)              # the frames whose whole span lies inside the signal


def many_minima_signal():
    i = np.arange(MANY['n'], dtype=np.float64)
    P = MANY['period']
    x = np.sin(2 * np.pi * i / P) + 0.4 * np.sin(6 * np.pi * i / P + 0.5) + 0.05 * np.sin(2 * np.pi * i / 57.3) + 1e-3 * np.sin(0.7391 * i * i)
    return (0.25 * x).astype(np.float32)


@functools.lru_cache(maxsize=None)
def many_minima_reference(n_cand):
    c = MANY
    return fr.candidates(many_minima_signal(), SR, c['hop'], c['W'], c['tau_min'], c['tau_max'], n_cand, 1.0)


# an exact tie: integers of period 12, W a multiple of the period: every d is an integer below 2^24 in either precision and
# d' is exactly zero at every multiple of the period
TIE = dict(W=48, hop=12, tau_min=5, tau_max=40, period=12, n=480)
TIE_PATTERN = (0, 3, 5, 2, -1, -4, -2, 1, 4, 6, 3, -3)


def tie_signal():
    return np.tile(np.array(TIE_PATTERN, np.float32), TIE['n'] // TIE['period'])


def tie_interior_frames():
    """Frames whose whole span lies inside the signal."""
    c = TIE
    F = fr.n_frames(c['n'], c['hop'])
    s = np.arange(F) * c['hop'] - (c['W'] + c['tau_max']) // 2
    return np.nonzero((s >= 0) & (s + c['W'] + c['tau_max'] + 1 <= c['n']))[0]


# a plateau: W = 1 makes d(k) = (x[s] - x[s + k])^2, so a frame's d' can be written down.  Frame 3 reads x[9 ..]:
# d = 0, 1, 1, 9, 0, 4, 4, 9 gives d' = 1, 1, 1, 27/11, 0, 4/3, 24/19, 9/4 (every product exact, every quotient of equal
# fractions equal in any precision): lag 1 (= tau_min) ties with lag 2 on its right and is a candidate (<=), lag 2 ties
# with lag 1 on its left and is not (<); lags 4 and 6 (= tau_max) are the other two.
PLATEAU = dict(W=1, hop=4, tau_min=1, tau_max=6, n_cand=3, ceiling=4.0, frame=3, lags=(1, 4, 6), n=40)


def plateau_signal():
    x = np.zeros(PLATEAU['n'], np.float32)
    x[9:17] = [0, 1, 1, 3, 0, 2, 2, 3]
    x[17:] = (np.arange(PLATEAU['n'] - 17) * 5 % 7)
    x[:9] = (np.arange(9) * 3 % 5)
    return x


LOG2_ULPS = 1.0       # the device library's log2f is documented to 1 ulp (ROCm device-libs, OCML); float64's is far below


def metrics_bound(ref, n):
    """A figure is the float32 rounding (half an ulp) of a float64 expression over n cells whose own relative error is at
    most a few n 2^-53: about one float32 ulp in all, as include/vc_hip.h says ("rounded to float32 once")."""
    ref = float(ref)
    return 0.5 * float(np.spacing(np.float32(abs(ref)))) * (1 + 1e-6) + 8.0 * n * 2.0 ** -53 * max(abs(ref), 1.0)


METRIC_CELLS = (255, 256, 257, 1000)


# ---------------------------------------------------------------------------------------------------- frame energy
def energy_tile(W, hop):
    G = 64
    while G > 1 and (W + (G - 1) * hop) * 4 > LDS_BUDGET:
        G >>= 1
    return G


# (W, hop): G = 64 four times, 16 and 1
ENERGY_CONFIGS = [(1, 1), (63, 7), (64, 64), (400, 80), (8192, 300), (65, 20000)]
ENERGY_TILES = [64, 64, 64, 64, 16, 1]


def energy_lengths(W, hop):
    G = energy_tile(W, hop)
    return [0, 1, hop - 1, hop, G * hop - 1, G * hop, G * hop + 1, G * hop + hop + 3]


def energy_rows(W, hop):
    lens = energy_lengths(W, hop)
    rng = np.random.RandomState(W + hop)
    base = (0.3 * rng.standard_normal(max(lens))).astype(np.float32)
    return [base[:n] for n in lens]


def energy_bound(W):
    """Relative: W non-negative float32 terms, ceil(W / 64) fused multiply-adds in a lane's chain and six levels of the
    butterfly."""
    k = -(-W // 64) + 6
    return k * EPS / (1.0 - k * EPS)


# ---------------------------------------------------------------------------------------------------- activity mask
MASK_FRAMES = (1, 2, 1023, 1024, 1025, 2048, 2049, 16384)       # frames per lane: 1 | 2 | 3 .. 16
MAX_GAP, MIN_RUN = 5, 4


def chunk(F):
    return -(-F // 1024)


def lane_pattern(F, max_gap=MAX_GAP, min_run=MIN_RUN):
    """A raw decision [F] with, where F has room: runs of min_run - 1 and of min_run frames at both ends, and across a lane
    boundary each a gap of max_gap, a gap of max_gap + 1, a run of min_run - 1 and a run of min_run frames."""
    m = np.zeros(F, bool)
    if F < 64:
        m[:] = [(f % 3) != 1 for f in range(F)]
        return m
    C = chunk(F)
    m[:min_run] = True                                                  # kept: min_run at the start ...
    m[F - (min_run - 1):] = True                                        # ... dropped: min_run - 1 at the end
    bounds = [C * k for k in range(1, F // C)]
    pick = [bounds[int(len(bounds) * q)] for q in (0.1, 0.25, 0.4, 0.55, 0.7, 0.85)]

    def run(lo, hi):
        m[lo:hi] = True

    b = pick[0]; run(b - 8, b - 2); run(b - 2 + max_gap, b + max_gap + 6)                  # a gap of max_gap over b
    b = pick[1]; run(b - 9, b - 3); run(b - 3 + max_gap + 1, b + max_gap + 6)              # a gap of max_gap + 1 over b
    b = pick[2]; run(b - 1, b - 1 + min_run - 1)                                           # min_run - 1 over b: dropped
    b = pick[3]; run(b - 2, b - 2 + min_run)                                               # min_run over b: kept
    b = pick[4]; run(b - 1, b); run(b + max_gap - 1, b + max_gap)                          # two single frames max_gap - 1 apart: kept only when the fill comes first
    b = pick[5]; run(b - 3 * max_gap, b + 3 * max_gap)
    return m


def mirrored(m):
    """The same pattern back to front: min_run - 1 at the start, min_run at the end."""
    return m[::-1].copy()


def energies_of(raw, rng):
    """Energies whose raw decision at ratio 1e-4 is `raw`: active frames in [0.5, 1], inactive ones zero or 1e-6."""
    if not raw.any():
        return np.zeros(len(raw), np.float32)
    e = np.where(raw, rng.uniform(0.5, 1.0, len(raw)), np.where(rng.rand(len(raw)) < 0.5, 0.0, 1e-6)).astype(np.float32)
    e[np.nonzero(raw)[0][0]] = 1.0
    return e


def raw_decision(e, ratio):
    """The header's raw decision on float32 energies, in float32."""
    e = np.asarray(e, np.float32)
    thr = np.float32(ratio) * (e.max() if len(e) else np.float32(0))
    return (e > 0) & (e > thr)


# ---------------------------------------------------------------------------------------------------- gain
GAIN_LENGTHS = (0, 1, 1023, 1024, 1025)
GAIN_HOPS = (80, 7)


def frame_of_sample(i, hop, F):
    return np.minimum((np.asarray(i) + hop // 2) // hop, F - 1)


def gain_bound():
    """The sums run in float64; the quotient is rounded to float32 once and the target is a float32: half an ulp and the
    sums' own n 2^-53.  tests/test_activity_gpu.py allows 2 eps; eps holds."""
    return EPS * (1 + 1e-6)
