"""Shape tables, input builders and bounds of tests/test_speaker_kernels_{cpu,gpu}.py: the launches of csrc/vc_gmm.hip, each
alone.  numpy only: tests/test_speaker_kernels_cpu.py proves every case usable without a device (the wrap cases wrap, the
exact cases are exact in the float64 reference, every bound holds the float32 restatement) and pins the bounds; the
reference is tests/speaker_ref.py.

The geometry the cases rely on is restated here from the header and the kernel file's comment: tiles of 32 frames, chunks
of 64 components, P(G) = max(1, 128 / G) partitions, tile k of utterance b in partition (b + k) mod P.

Every reference is computed once per process (functools.lru_cache) and never modified by a test."""
import fractions
import functools

import numpy as np

import speaker_ref as sr

EPS = 2.0 ** -24                      # the unit round-off of float32
U64 = 2.0 ** -53                      # and of float64
TILE, CHUNK, PARTS, LANES = 32, 64, 128, 256
MAX_M, MAX_D, MAX_G = 256, 64, 4096
PAD = 3                               # max_frames = the longest utterance + 3: NaN rows behind every utterance


# ---------------------------------------------------------------------------------------------------- geometry
def partitions(G):
    return 1 if G >= PARTS else PARTS // G


def n_tiles(n):
    return -(-max(int(n), 0) // TILE)


def partition_of(b, k, P):
    return (b + k) % P


def walk(lens, groups, G):
    """{(g, p): [(b, k), ...]} in the order workgroup (., p, g) takes them: utterances ascending, of each its tiles
    k = first, first + P, ... with first = (p - b mod P + P) mod P."""
    P = partitions(G)
    out = {}
    for g in range(G):
        for p in range(P):
            todo = []
            for b, n in enumerate(lens):
                if groups[b] != g:
                    continue
                k = (p - b % P + P) % P
                while k < n_tiles(n):
                    todo.append((b, k))
                    k += P
            if todo:
                out[(g, p)] = todo
    return out


def wrapped(lens, groups, G):
    """The (b, k) a partition reaches by its SECOND or later step through utterance b: the tiles `k += P` produces."""
    out = []
    for todo in walk(lens, groups, G).values():
        seen = set()
        for b, k in todo:
            if b in seen:
                out.append((b, k))
            seen.add(b)
    return sorted(out)


def workspace_bytes(G, M, D):
    P = partitions(G)
    if P == 1:
        return 0
    return (G * P * -(-M // CHUNK) * (CHUNK * (1 + 2 * D) + 1) * 8 + 255) // 256 * 256


def table_floats(S, M, D):
    return (S + 1) * M * D + M


# ---------------------------------------------------------------------------------------------------- exact mixtures
def exact_model(M, m_star, D, n_models=1, seed=0):
    """One live component m_star (weight 1, every other weight 0), integer means in [-2, 2] that differ between the models
    in the live component, variances 1: gamma is exactly 1 for m_star and exactly 0 elsewhere."""
    rng = np.random.RandomState(1000 * M + 10 * D + m_star + seed)
    w = np.zeros(M, np.float32)
    w[m_star] = 1.0
    mu = rng.randint(-2, 3, (n_models, M, D)).astype(np.float32)
    for s in range(n_models):
        mu[s, m_star, 0] = (s % 5) - 2
    return w, mu, np.ones((M, D), np.float32)


def int_features(rng, lens, D, max_frames=None):
    """[B, max_frames, D] small integers below each length, NaN behind it."""
    F = max(max(lens), 1) + PAD if max_frames is None else max_frames
    x = np.full((len(lens), F, D), np.nan, np.float32)
    for b, n in enumerate(lens):
        n = min(max(n, 0), F)
        x[b, :n] = rng.randint(-3, 4, (n, D))
    return x


def random_mask(rng, lens, F, keep=0.7):
    """uint8 [B, F]: random below each length, SET behind it (a frame behind the length is never kept, whatever its byte)."""
    m = np.full((len(lens), F), 0xA5, np.uint8)
    for b, n in enumerate(lens):
        n = min(max(n, 0), F)
        m[b, :n] = rng.rand(n) < keep
    return m


def kept(lens, F, mask=None):
    k = np.zeros((len(lens), F), bool)
    for b, n in enumerate(lens):
        k[b, :min(max(n, 0), F)] = True
    return k if mask is None else k & (np.asarray(mask) != 0)


def exact_ll(c_table, x, mu_live):
    """float32(c - q / 2), q the integer sum of (x - mu)^2: what fmaf(-0.5, q, c) gives, and -- the sum of the exponentials
    being exactly 1 -- the frame's ll."""
    q = ((np.asarray(x, np.float64) - np.asarray(mu_live, np.float64)) ** 2).sum(-1)
    return (np.float64(np.float32(c_table)) - 0.5 * q).astype(np.float32)


def exact_sums(x, lens, groups, G, M, m_star, mask=None):
    """The integer statistics of an exact case: N[g, m*] = the kept frames of the group, S1 = sum x, S2 = sum x^2, every
    other component 0; and keep [B, F]."""
    B, F, D = x.shape
    keep = kept(lens, F, mask)
    N, S1, S2 = np.zeros((G, M)), np.zeros((G, M, D)), np.zeros((G, M, D))
    for b in range(B):
        g = int(groups[b])
        if not 0 <= g < G:
            continue
        xb = x[b][keep[b]].astype(np.int64)
        N[g, m_star] += len(xb)
        S1[g, m_star] += xb.sum(0)
        S2[g, m_star] += (xb * xb).sum(0)
    return N, S1, S2, keep


def l_bound(n):
    """L is a float64 sum of n float32 terms: relative to the sum of their magnitudes."""
    return n * U64


# ---------------------------------------------------------------------------------------------------- accumulate
# name: G, (M, m_star, D), lens, groups, mask?; `wrap` / `b_ge_p`: what the CPU file must find in the case
IFILL = 0x7FFFFFFF
ACC_EXACT = {
    'wrap_p2': dict(G=64, shape=(1, 0, 2), lens=[65], groups=[7], mask=False, wrap=True),
    'wrap_p3': dict(G=42, shape=(64, 63, 5), lens=[129], groups=[41], mask=True, wrap=True),
    'wrap_p42': dict(G=3, shape=(65, 64, 3), lens=[1345], groups=[2], mask=True, wrap=True),
    'wrap_p128': dict(G=1, shape=(2, 1, 2), lens=[4097], groups=[0], mask=True, wrap=True),
    'b_ge_p2': dict(G=64, shape=(65, 64, 4), lens=[33, 1, 70, 32, 97], groups=[0, 63, 0, 63, 0], mask=True, wrap=True, b_ge_p=True),
    'b_ge_p128': dict(G=1, shape=(256, 255, 1), lens=[1 + b % 3 for b in range(130)], groups=[0] * 130, mask=False, b_ge_p=True),
    'z_limit': dict(G=4096, shape=(1, 0, 1), lens=[33, 5, 64, 1, 40, 2], groups=[0, 4095, 17, 4095, -1, 2048], mask=True),
    'left_out': dict(G=3, shape=(64, 0, 4), lens=[40, 33, 7, 64, 12], groups=[0, -1, 3, IFILL, 2], mask=True),      # group 1: no utterance
    'model_0_of_3': dict(G=3, shape=(65, 64, 5), lens=[40, 33, 7], groups=[0, 2, 0], mask=True, n_models=3, model=0),
    'model_2_of_3': dict(G=3, shape=(65, 64, 5), lens=[40, 33, 7], groups=[0, 2, 0], mask=True, n_models=3, model=2),
}
ACC_MS, ACC_DS = (1, 64, 65, 256), (1, 4, 5, 63, 64)
for _M in ACC_MS:
    for _D in ACC_DS:
        ACC_EXACT['own_M%d_D%d' % (_M, _D)] = dict(G=3, shape=(_M, _M - 1, _D), lens=[1, 33, 40], groups=[2, 0, 2], mask=True)
# the workspace path against the direct path: the same inputs, groups in [0, 64), at G and G + 1
ACC_PAIRS = ((64, 65), (127, 128))
ACC_PAIR_CASE = dict(shape=(65, 63, 5), lens=[70, 1, 33, 64, 97], groups=[0, 63, 5, 63, 0], mask=True)


@functools.lru_cache(maxsize=None)
def acc_exact(name, G=None):
    """The inputs of an exact case (dirty: NaN features behind every length, set mask bytes there) and its integer sums."""
    c = dict(ACC_PAIR_CASE if name == 'pair' else ACC_EXACT[name])
    G = c.get('G', G)
    M, m_star, D = c['shape']
    S, model = c.get('n_models', 1), c.get('model', 0)
    rng = np.random.RandomState(sum(map(ord, name)))
    w, mu, var = exact_model(M, m_star, D, S)
    x = int_features(rng, c['lens'], D)
    F = x.shape[1]
    mask = random_mask(rng, c['lens'], F) if c['mask'] else None
    N, S1, S2, keep = exact_sums(x, c['lens'], c['groups'], G, M, m_star, mask)
    return dict(name=name, G=G, M=M, m_star=m_star, D=D, S=S, model=model, lens=list(c['lens']), groups=list(c['groups']), w=w, mu=mu,
                var=var, x=x, F=F, mask=mask, keep=keep, N=N, S1=S1, S2=S2)


def clean(x):
    """The features with zeros for NaN: what the float64 reference is given (it slices below the lengths anyway)."""
    return np.nan_to_num(np.asarray(x), nan=0.0, posinf=0.0, neginf=0.0)


def order_bound(frames, P, abs_sum):
    """Workspace path against direct path: the same float64 terms in another order, (frames + P) roundings at most."""
    return (frames + P) * U64 * abs_sum


# the documented order of the float64 additions, observable in N alone (plain additions: nothing a compiler may fuse):
# P = 3; utterance 0 has four tiles (partitions 0 1 2 0), utterance 1 two (partitions 1 2), another group one utterance
ORDER_CASE = dict(G=42, D=2, M=64, lens=[100, 45, 70], groups=[0, 0, 41])


def ordered_sum(gamma, keep, lens, groups, G):
    """N [G, M] as the header orders it: a partition walks its utterances and tiles ascending and adds frame by frame from
    0.0; the P partial sums meet in the order 0 .. P - 1 from 0.0 (one partition: its sum is the output).  gamma [B, F, M]
    float64, keep [B, F]."""
    P = partitions(G)
    todo = walk(lens, groups, G)
    out = np.zeros((G, gamma.shape[2]))
    for g in range(G):
        parts = []
        for p in range(P):
            s = np.zeros(gamma.shape[2])
            for b, k in todo.get((g, p), []):
                for f in range(k * TILE, min((k + 1) * TILE, lens[b])):
                    if keep[b, f]:
                        s = s + gamma[b, f]
            parts.append(s)
        if P == 1:
            out[g] = parts[0]
        else:
            acc = np.zeros(gamma.shape[2])
            for s in parts:
                acc = acc + s
            out[g] = acc
    return out


# the real-valued case of tests/test_speaker_gpu.py (hard_case: a narrow component, a frame 40 sigma out), with a mask
ACC_REAL = [(8, 65, 1), (8, 65, 3), (5, 256, 64), (63, 64, 128)]            # (D, M, G)
REAL_LENS = [1, 31, 32, 33, 70, 50]


@functools.lru_cache(maxsize=None)
def real_case(D, M, n_models=2):
    from test_speaker_cpu import hard_case
    x70, w, mu, var = hard_case(D, M, 70, seed=1000 * D + M)
    rng = np.random.RandomState(D * 7 + M)
    F = 70 + PAD
    x = np.full((len(REAL_LENS), F, D), np.nan, np.float32)
    for b, n in enumerate(REAL_LENS):
        x[b, :n] = x70[:n] if n == 70 else x70[rng.randint(0, 69, n)]
    mus = np.stack([mu] + [(mu + 0.2 * rng.standard_normal(mu.shape)).astype(np.float32) for _ in range(n_models - 1)])
    mask = random_mask(rng, REAL_LENS, F, 0.8)
    return dict(x=x, lens=list(REAL_LENS), w=w, mu=mus, var=var, F=F, mask=mask, D=D, M=M)


@functools.lru_cache(maxsize=None)
def real_ll(D, M, model=0, n_models=2):
    """Per utterance (ll float64 [n], frame_bound [n]) under one model of real_case."""
    c = real_case(D, M, n_models)
    out = []
    for b, n in enumerate(c['lens']):
        ll, E = sr.loglik(c['x'][b, :n], c['w'], c['mu'][model], c['var'])
        out.append((ll, sr.frame_bound(D, M, E)))
    return out


# ---------------------------------------------------------------------------------------------------- features
FEAT_LENS = [-5, 0, 1, 2, 3, 4, 5, 257, 257 + PAD + 100]       # max_frames = 257 + PAD: the last one is clamped to it
FEAT_FRAMES = 257 + PAD
FEAT_COEF = (1, 31, 32)


def feat_eff(n, F=FEAT_FRAMES):
    return min(max(n, 0), F)


@functools.lru_cache(maxsize=None)
def feat_batch(n_coef, integer=False, seed=0):
    """cep [B, F, n_coef] with NaN rows behind every (clamped) length; mask [B, F] random below, set behind."""
    rng = np.random.RandomState(50 * n_coef + integer + seed)
    B, F = len(FEAT_LENS), FEAT_FRAMES
    cep = np.full((B, F, n_coef), np.nan, np.float32)
    for b, n in enumerate(FEAT_LENS):
        e = feat_eff(n)
        cep[b, :e] = rng.randint(-8, 9, (e, n_coef)) if integer else 3.0 * rng.standard_normal((e, n_coef))
    return cep, random_mask(rng, FEAT_LENS, F)


def feat_bound(A):
    """test_features_against_float64 of tests/test_speaker_gpu.py: 8 u A, A the largest |cepstrum| of the utterance."""
    return 8.0 * EPS * A


ONE_KEPT = (12, 13, 14, 15)           # one kept frame in each of the lanes r = f mod 4 = 0 .. 3


# ---------------------------------------------------------------------------------------------------- prepare
PREP_SHAPES = [(1, 1, 1), (2, 63, 3), (5, 65, 64), (1, 256, 64),
               (1, 85, 1), (2, 64, 1), (3, 1, 64), (1, 7, 36), (2, 128, 1), (1, 27, 9)]       # (n_models, M, D)
PREP_SEAMS = [255, 256, 257, 511, 512, 513]                                                   # table floats of the last six


@functools.lru_cache(maxsize=None)
def prep_model(S, M, D, zero_weight=None):
    rng = np.random.RandomState(S + 7 * M + 13 * D)
    w = rng.dirichlet(np.full(M, 3.0)).astype(np.float32)
    if zero_weight is not None:
        w[zero_weight] = 0.0
    mu = rng.standard_normal((S, M, D)).astype(np.float32)
    var = np.exp(rng.uniform(np.log(1e-4), np.log(50.0), (M, D))).astype(np.float32)
    return w, mu, var


def c_reference(w, var):
    """(c_m float64, its bound): half a float32 ulp of the result plus (D + 2) 2^-53 sum |terms| -- D + 1 additions and
    the product by 0.5 in float64, each logarithm within an ulp of its own magnitude (the device's float64 log may differ
    from numpy's in the last bit)."""
    w64, v64 = np.asarray(w, np.float64), np.asarray(var, np.float64)
    with np.errstate(divide='ignore'):
        lw = np.log(w64)
    terms = np.log(2.0 * np.pi * v64)
    c = lw - 0.5 * terms.sum(1)
    D = v64.shape[1]
    with np.errstate(invalid='ignore'):
        mag = np.where(np.isfinite(lw), np.abs(lw), 0.0) + np.abs(terms).sum(1)
        ulp = np.where(np.isfinite(c), np.spacing(np.abs(c).astype(np.float32)).astype(np.float64), 0.0)
    return c, 0.5 * ulp * (1 + 1e-6) + (D + 2) * U64 * mag


# ---------------------------------------------------------------------------------------------------- loglik
LL_LENS = [0, 1, 7, 8, 9, 31, 32, 33, 70]
LL_FRAMES = (33, 70)
LL_MS = (1, 63, 64, 65, 128, 129, 192, 193, 255, 256)
LL_DS = (1, 63, 64)
LL_MODELS = (1, 2, 5)


def ll_model_index(S):
    """d_model for the nine utterances of LL_LENS: -3, 0, S - 1, S + 5 and again; what the clamp makes of them."""
    raw = [(-3, 0, S - 1, S + 5)[b % 4] for b in range(len(LL_LENS))]
    return raw, [min(max(v, 0), S - 1) for v in raw]


@functools.lru_cache(maxsize=None)
def ll_case(D, M, S=2, max_frames=70):
    """Nine utterances of hard_case frames (utterance 8: the 70 frames themselves, with the narrow component's frames and
    the frame 40 sigma out), clamped to max_frames, NaN behind."""
    c = real_case(D, M, 2)
    from test_speaker_cpu import hard_case
    x70 = hard_case(D, M, 70, seed=1000 * D + M)[0]
    rng = np.random.RandomState(3 * D + M + S)
    mus = np.stack([c['mu'][0]] + [(c['mu'][0] + 0.2 * rng.standard_normal(c['mu'][0].shape)).astype(np.float32) for _ in range(S - 1)])
    x = np.full((len(LL_LENS), max_frames, D), np.nan, np.float32)
    for b, n in enumerate(LL_LENS):
        e = min(n, max_frames)
        x[b, :e] = x70[:e] if n == 70 else x70[rng.randint(0, 70, e)]
    return dict(x=x, lens=list(LL_LENS), eff=[min(n, max_frames) for n in LL_LENS], w=c['w'], mu=mus, var=c['var'], F=max_frames, D=D, M=M, S=S)


# ---------------------------------------------------------------------------------------------------- score
SCORE_LENS = [0, 1, 255, 256, 257, 513]
SCORE_FRAMES = 513 + PAD


@functools.lru_cache(maxsize=None)
def score_batch(integer):
    rng = np.random.RandomState(40 + integer)
    B, F = len(SCORE_LENS), SCORE_FRAMES
    a, b_ = np.full((B, F), np.nan, np.float32), np.full((B, F), np.nan, np.float32)
    for u, n in enumerate(SCORE_LENS):
        a[u, :n] = rng.randint(-90, -20, n) if integer else -40.0 + 9.0 * rng.standard_normal(n)
        b_[u, :n] = rng.randint(-90, -20, n) if integer else a[u, :n] - 0.4 + 0.3 * rng.standard_normal(n)
    return a, b_, random_mask(rng, SCORE_LENS, F, 0.6)


def score_bound(ref, n, scale=None):
    """metrics_bound of tests/score_kernels_cases.py: half a float32 ulp of the figure plus the float64 sum's n 2^-53,
    relative to `scale` (the mean magnitude of the terms; for the difference, of both means)."""
    ref = float(ref)
    scale = abs(ref) if scale is None else scale
    return 0.5 * float(np.spacing(np.float32(abs(ref)))) * (1 + 1e-6) + n * U64 * max(scale, 1.0)


# ---------------------------------------------------------------------------------------------------- update
UPDATE_EM_SHAPES = [(85, 3), (64, 4), (43, 6), (256, 64)]     # M D = 255, 256, 258 and the largest.  257 is a prime above both
UPDATE_MAP_257 = (257, 1, 1)                                  # limits (M <= 256, D <= 64): no M D equals it; G M D = 257 does, in MAP
UPDATE_ULPS = 2.0                                             # test_update_em_and_map_against_the_reference


@functools.lru_cache(maxsize=None)
def update_stats(G, M, D, seed=0):
    rng = np.random.RandomState(G + 3 * M + 11 * D + seed)
    N = rng.uniform(2.0, 50.0, (G, M))
    mean = rng.standard_normal((G, M, D))
    v = rng.uniform(0.2, 2.0, (G, M, D))
    mu_old = rng.standard_normal((M, D)).astype(np.float32)
    var_old = rng.uniform(0.5, 1.5, (M, D)).astype(np.float32)
    return N, mean, v, mu_old, var_old


def cancellation_case():
    """n, S1, S2 (float64) of one component whose variance (1e-3) lies far below its squared mean (1e6)."""
    n, mean, var = 37.25, 1000.0 + 1.0 / 3.0, 1e-3
    return n, mean * n, (var + mean * mean) * n


def cancellation_bound(n, S1, S2):
    """Half a float32 ulp of the variance plus 4 2^-53 (S2 / n + mean^2): the two quotients, the product and the
    subtraction (or the one rounding of a fused multiply-add) each round a value no larger than S2 / n or mean^2."""
    n, S1, S2 = (fractions.Fraction(v) for v in (n, S1, S2))
    true = S2 / n - (S1 / n) ** 2
    return float(true), 0.5 * float(np.spacing(np.float32(float(true)))) * (1 + 1e-6) + 4 * U64 * float(S2 / n + (S1 / n) ** 2)


def variance_float64(n, S1, S2, fused):
    """The kernel's float64 expression S2 / n - mean * mean, with the subtraction contracted into one fused multiply-add
    (fused) or not: a compiler may do either."""
    mean, e2 = S1 / n, S2 / n
    if not fused:
        return e2 - mean * mean
    return float(fractions.Fraction(e2) - fractions.Fraction(mean) * fractions.Fraction(mean))
