"""The resampler's definition (include/vc_hip.h, "Resampling") written directly in numpy -- not a test module.

    y[m] = sum_{0 <= n < len} x[n] * h((m * down - n * up) / up),   0 <= m < ceil(len * up / down)
    h(t) = fc * sinc(fc t) * I0(beta * sqrt(1 - u^2)) / I0(beta),  u = t * fc / Z,  |u| < 1, else 0

``dtype=np.float64`` is the reference.  ``dtype=np.float32`` rounds the taps and the samples to float32 and accumulates
product by product, one tap after the other in ascending k (a float32 multiply, then a float32 add: no pairwise
summation, no fused multiply-add): its distance from the float64 run is the yardstick for the device's error.
The taps are computed here from the closed form, independently of audio_lib.resample_taps."""
import math

import numpy as np
from scipy import special

PRESETS = {'kaiser_best': (64, 0.9475937167399596, 14.769656459379492),
           'kaiser_fast': (16, 0.85, 8.555504641634386)}


def h_closed(t, fc, Z, beta):
    """h(t) for one float t (input samples), straight from the formula."""
    u = t * fc / Z
    if abs(u) >= 1.0:
        return 0.0
    x = fc * t
    s = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
    return fc * s * float(special.i0(beta * math.sqrt(1.0 - u * u))) / float(special.i0(beta))


def ratio(sr_in, sr_out):
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def taps(sr_in, sr_out, res_type='kaiser_best'):
    """(up, down, half, g float64 [2 * half + 1]) with g[k + half] = h(k / up)."""
    Z, rolloff, beta = PRESETS[res_type] if isinstance(res_type, str) else res_type
    up, down = ratio(sr_in, sr_out)
    fc = rolloff * min(1.0, up / down)
    half = int(math.ceil(Z * up / fc)) - 1
    k = np.arange(-half, half + 1, dtype=np.float64)
    t = k / up
    u2 = (t * fc / Z) ** 2
    ok = u2 < 1.0
    g = np.zeros_like(t)
    g[ok] = fc * np.sinc(fc * t[ok]) * special.i0(beta * np.sqrt(1.0 - u2[ok])) / special.i0(beta)
    return up, down, half, g


def out_len(n, sr_in, sr_out):
    up, down = ratio(sr_in, sr_out)
    return (int(n) * up + down - 1) // down


def resample(x, sr_in, sr_out, res_type='kaiser_best', dtype=np.float64):
    """The sum above for one utterance x [len]; returns ``dtype`` [ceil(len * up / down)].  Vectorised over the outputs,
    sequential over the taps: acc += x[n] * g[k] for k = m * down - n * up ascending (n descending)."""
    up, down, half, g = taps(sr_in, sr_out, res_type)
    x = np.asarray(x, dtype=np.float64).astype(dtype)
    g = g.astype(dtype)
    n_in = len(x)
    n_out = (n_in * up + down - 1) // down
    m = np.arange(n_out, dtype=np.int64)
    q, p = np.divmod(m * down, up)                  # m * down = q * up + p;  k = p + j * up,  n = q - j
    acc = np.zeros(n_out, dtype=dtype)
    for j in range(-((half + up - 1) // up), half // up + 1):
        k = p + j * up
        n = q - j
        ok = (np.abs(k) <= half) & (n >= 0) & (n < n_in)
        prod = x[np.where(ok, n, 0)] * g[np.where(ok, k + half, 0)]          # rounded to dtype
        acc = acc + np.where(ok, prod, dtype(0))                              # rounded to dtype
    return acc


def distance(a, ref):
    """(max |a - ref| / max |ref|, ||a - ref||_2 / ||ref||_2) in float64."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = a - ref
    return float(np.abs(d).max() / np.abs(ref).max()), float(np.sqrt((d * d).sum() / (ref * ref).sum()))
