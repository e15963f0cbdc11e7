"""Shapes and inputs of the exemplar-conversion tests, shared by tests/test_exemplar_cpu.py (which proves them usable on the
restatement) and tests/test_exemplar_gpu.py."""
import numpy as np

import exemplar_ref as er

KEY_CLASSES = (1, 61, 64, 65, 128)
KEY_LENS = [0, 1, 5, 9, 3]                              # a ragged batch with an empty utterance; F = 9 + PAD
PAD = 2
SEAM_MQ = (1, 15, 16, 17, 33, 65)
SEAM_N = (1, 15, 16, 17, 63, 64, 65, 1000)
SEAM_K = (1, 4, 16)
SEAM_SPLITS = (1, 2, 3, 7, 0)
MEAN_DIMS = (1, 63, 64, 65, 80, 201)
MAX_DOT_128 = 128 * 127 * 127                           # the all-127 key at Kp = 128 against itself: 2,064,512
D_MAX = 2 * MAX_DOT_128                                 # ... against the zero key: the greatest distance, 4,129,024


def half_points():
    """float32 values p whose 127 * sqrtf(p), computed in float32, is exactly m + 0.5: [(p, m)] for as many m in 0 .. 126 as
    have one among the floats next to ((m + 0.5) / 127)^2.  rintf must take them to the even neighbour."""
    out = []
    for m in range(127):
        p = np.float32(((m + 0.5) / 127.0) ** 2)
        for _ in range(8):
            p = np.nextafter(p, np.float32(0))
        for _ in range(17):
            if np.float32(127.0) * np.sqrt(p) == np.float32(m + 0.5):
                out.append((p, m))
                break
            p = np.nextafter(p, np.float32(2))
    return out


def edge_values():
    """(values float32, expected keys): the quantiser's edges."""
    tiny = np.float32(1.0 / (254.0 * 254.0))            # 127 sqrt(p) = 0.5: rounds to 0 (even)
    vals = [0.0, -0.0, 1e-45, 1e-40, 1.1754944e-38, float(tiny), float(np.nextafter(tiny, np.float32(1))), 1.0,
            float(np.nextafter(np.float32(1), np.float32(0))), 2.0, np.inf, np.nan, -1e-3, -1.0, -np.inf, 0.25, 0.5]
    want = [0, 0, 0, 0, 0, None, None, 127, 127, 127, 127, 0, 0, 0, 0, None, None]
    hp = half_points()
    vals += [float(p) for p, _ in hp]
    want += [m if m % 2 == 0 else m + 1 for _, m in hp]
    return np.array(vals, np.float32), want


def key_case(C, seed=0):
    """(ppg [B, F, C] with NaN rows beyond the lengths and the edge values sprinkled over the live rows, n_frames)."""
    rng = np.random.RandomState(10 + C + seed)
    B, F = len(KEY_LENS), max(KEY_LENS) + PAD
    z = rng.standard_normal((B, F, C)) * 3.0
    p = np.exp(z - z.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    edges = edge_values()[0]
    flat = p.reshape(-1)
    at = rng.permutation(flat.size)[:min(len(edges), flat.size)]
    flat[at] = edges[:len(at)]
    for b, n in enumerate(KEY_LENS):
        p[b, n:] = np.nan
    return p, np.array(KEY_LENS, np.int32)


def random_keys(n, Kp, seed, C=None):
    """n asymmetric keys over the full range 0 .. 127 (the columns at or beyond C zero) and their norms."""
    rng = np.random.RandomState(seed)
    key = rng.randint(0, 128, (n, Kp)).astype(np.int8)
    key *= (rng.rand(n, Kp) < 0.7).astype(np.int8)       # zeros too: norms differ widely
    if C is not None:
        key[:, C:] = 0
    return key, (key.astype(np.int32) ** 2).sum(1).astype(np.int32)


def clustered_keys(n, Kp, seed, n_centres=5):
    """Keys that repeat: many equal distances, so the (d, j) order is exercised."""
    rng = np.random.RandomState(seed)
    centres, _ = random_keys(n_centres, Kp, seed + 1)
    key = centres[rng.randint(0, n_centres, n)]
    return key, (key.astype(np.int32) ** 2).sum(1).astype(np.int32)


def sorted_bank(n, Kp, descending):
    """A query and a bank whose distance to it strictly ascends (descends) with the row: the query is e_0 * 127, bank row j is
    e_0 * (127 - j') with j' = j or n - 1 - j, so d = j'^2."""
    assert n <= 128
    q = np.zeros((1, Kp), np.int8)
    q[0, 0] = 127
    bank = np.zeros((n, Kp), np.int8)
    order = np.arange(n)[::-1] if descending else np.arange(n)
    bank[:, 0] = 127 - order
    norm = lambda k: (k.astype(np.int32) ** 2).sum(1).astype(np.int32)
    return q, norm(q), bank, norm(bank)


def mean_case(Mq, k, N, D, seed=0):
    """(idx, dist [Mq, k] sorted lists with -1 tails of every length, one row without a filled slot; values [N, D])."""
    rng = np.random.RandomState(50 + seed + D + k)
    idx = rng.randint(0, N, (Mq, k)).astype(np.int32)
    dist = np.sort(rng.randint(1, 5000, (Mq, k)), axis=1).astype(np.int32)
    for m in range(Mq):
        n = m % (k + 1)                                 # filled slots: 0 .. k
        idx[m, n:], dist[m, n:] = -1, -1
    V = rng.standard_normal((N, D)).astype(np.float32)
    V[0, 0] = -0.0
    return idx, dist, V
