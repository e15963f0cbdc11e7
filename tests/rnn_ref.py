"""Float64 definitions of the recurrent and row-wise inference kernels (csrc/vc_rnn.hip; contracts in include/vc_hip.h),
plain numpy, nothing imported from the package.

  gru_bidir        vc_gru_bidir: g = sigmoid(xg + h Wg_h); r, u = split(g), r FIRST; c = tanh(xc + (r h) Wc_h);
                   h' = u h + (1 - u) c; zero initial state; the backward direction runs t = T-1 .. 0.
                   xproj [n_seq T, 6H] = (gates 2H | candidate H) of fw, then of bw; Wh [H, 3H] = [Wg_h | Wc_h]
  lstm_bidir       vc_lstm_bidir: z = x-part + h Wh; i, j, f, o = split(z); c' = sigmoid(f + 1) c + sigmoid(i) tanh(j);
                   h' = sigmoid(o) tanh(c'); xproj [n_seq T, 8H] (fw 4H | bw 4H); Wh [H, 4H]
  softmax_argmax   vc_softmax_argmax: softmax over the last axis; the FIRST maximum's index
  to_bf16          float32 -> bf16, round to nearest even, returned as the float32 numbers on the bf16 grid
                   (to_bf16_bits: the 16 bits)

Restatements: the same operations in float32, rounding where a kernel rounds.  They are used ONLY to size error bounds
(a test allows a multiple of the restatement's own distance from float64 on the same input), never as expected values.

  gru_bidir_f32(.., bf16_state)  bf16_state = False: h and r h stay float32 in the matrix products (gru_wave_kernel,
                   gru_generic_kernel, gru_resident_kernel with float32 weights); True: both are rounded to bf16 in
                   front of the products, the state update itself stays float32 (gru_resident_kernel with bf16
                   weights, gru_mfma_kernel)
  lstm_bidir_f32   float32 throughout (lstm_generic_kernel)
  softmax_f32      float32 exp(x - max), float32 sum, one reciprocal, one product
  out_bf16 = True rounds what is returned to bf16, as out_dtype = VC_BF16 does.

Everything returned is a float64 numpy array (class ids: int64); activations are [n_seq T, C] as the library takes them.
"""
import numpy as np

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------ bf16

def to_bf16_bits(x):
    """float32 -> the 16 bits of its bf16 rounding (nearest, ties to even; NaN stays a quiet NaN of the same sign)."""
    b = np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32).astype(np.uint64)
    nan = ((b & 0x7f800000) == 0x7f800000) & ((b & 0x007fffff) != 0)
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    r = np.where(nan, (b >> 16) | 0x0040, r)
    return r.astype(np.uint16)


def from_bf16_bits(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def to_bf16(x):
    x = np.asarray(x, dtype=F32)
    return from_bf16_bits(to_bf16_bits(x)).reshape(x.shape)


# ------------------------------------------------------------------------------------------ float64 definitions

def _sigmoid(v):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-v))


def _order(T, reverse):
    return range(T - 1, -1, -1) if reverse else range(T)


def gru_direction(xp, wh, T, reverse):
    """xp [n_seq T, 3H] (gates 2H | candidate H), wh [H, 3H] -> [n_seq T, H]."""
    xp, wh = np.asarray(xp, F64), np.asarray(wh, F64)
    H = wh.shape[0]
    x = xp.reshape(-1, T, 3 * H)
    h = np.zeros((x.shape[0], H), F64)
    out = np.empty((x.shape[0], T, H), F64)
    for t in _order(T, reverse):
        g = _sigmoid(x[:, t, :2 * H] + h @ wh[:, :2 * H])
        r, u = g[:, :H], g[:, H:]
        c = np.tanh(x[:, t, 2 * H:] + (r * h) @ wh[:, 2 * H:])
        h = u * h + (1.0 - u) * c
        out[:, t] = h
    return out.reshape(-1, H)


def gru_bidir(xproj, wh_fw, wh_bw, T):
    H = np.asarray(wh_fw).shape[0]
    xproj = np.asarray(xproj, F64)
    return np.concatenate([gru_direction(xproj[:, :3 * H], wh_fw, T, False),
                           gru_direction(xproj[:, 3 * H:], wh_bw, T, True)], axis=1)


def lstm_direction(xp, wh, T, reverse):
    """xp [n_seq T, 4H] (i | j | f | o), wh [H, 4H] -> [n_seq T, H]."""
    xp, wh = np.asarray(xp, F64), np.asarray(wh, F64)
    H = wh.shape[0]
    x = xp.reshape(-1, T, 4 * H)
    h = np.zeros((x.shape[0], H), F64)
    c = np.zeros_like(h)
    out = np.empty((x.shape[0], T, H), F64)
    for t in _order(T, reverse):
        z = x[:, t] + h @ wh
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c = _sigmoid(f + 1.0) * c + _sigmoid(i) * np.tanh(j)
        h = _sigmoid(o) * np.tanh(c)
        out[:, t] = h
    return out.reshape(-1, H)


def lstm_bidir(xproj, wh_fw, wh_bw, T):
    H = np.asarray(wh_fw).shape[0]
    xproj = np.asarray(xproj, F64)
    return np.concatenate([lstm_direction(xproj[:, :4 * H], wh_fw, T, False),
                           lstm_direction(xproj[:, 4 * H:], wh_bw, T, True)], axis=1)


def softmax_argmax(logits):
    """[M, N] -> (probabilities [M, N] float64, class ids [M] int64: the first maximum)."""
    x = np.asarray(logits, F64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True), np.argmax(x, axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------ float32 restatements

def _sigmoid32(v):
    with np.errstate(over='ignore'):
        return (F32(1) / (F32(1) + np.exp(-v))).astype(F32)


def _gru_direction_f32(xp, wh, T, reverse, bf16_state):
    xp, wh = np.asarray(xp, F32), np.asarray(wh, F32)
    H = wh.shape[0]
    x = xp.reshape(-1, T, 3 * H)
    q = to_bf16 if bf16_state else (lambda a: a)
    h = np.zeros((x.shape[0], H), F32)
    out = np.empty((x.shape[0], T, H), F32)
    for t in _order(T, reverse):
        g = _sigmoid32(x[:, t, :2 * H] + q(h) @ wh[:, :2 * H])
        r, u = g[:, :H], g[:, H:]
        c = np.tanh(x[:, t, 2 * H:] + q(r * h) @ wh[:, 2 * H:]).astype(F32)
        h = (u * h + (F32(1) - u) * c).astype(F32)
        out[:, t] = h
    return out.reshape(-1, H)


def gru_bidir_f32(xproj, wh_fw, wh_bw, T, bf16_state=False, out_bf16=False):
    H = np.asarray(wh_fw).shape[0]
    xproj = np.asarray(xproj, F32)
    y = np.concatenate([_gru_direction_f32(xproj[:, :3 * H], wh_fw, T, False, bf16_state),
                        _gru_direction_f32(xproj[:, 3 * H:], wh_bw, T, True, bf16_state)], axis=1)
    return (to_bf16(y) if out_bf16 else y).astype(F64)


def _lstm_direction_f32(xp, wh, T, reverse):
    xp, wh = np.asarray(xp, F32), np.asarray(wh, F32)
    H = wh.shape[0]
    x = xp.reshape(-1, T, 4 * H)
    h = np.zeros((x.shape[0], H), F32)
    c = np.zeros_like(h)
    out = np.empty((x.shape[0], T, H), F32)
    for t in _order(T, reverse):
        z = (x[:, t] + h @ wh).astype(F32)
        i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        c = (_sigmoid32(f + F32(1)) * c + _sigmoid32(i) * np.tanh(j)).astype(F32)
        h = (_sigmoid32(o) * np.tanh(c)).astype(F32)
        out[:, t] = h
    return out.reshape(-1, H)


def lstm_bidir_f32(xproj, wh_fw, wh_bw, T, out_bf16=False):
    H = np.asarray(wh_fw).shape[0]
    xproj = np.asarray(xproj, F32)
    y = np.concatenate([_lstm_direction_f32(xproj[:, :4 * H], wh_fw, T, False),
                        _lstm_direction_f32(xproj[:, 4 * H:], wh_bw, T, True)], axis=1)
    return (to_bf16(y) if out_bf16 else y).astype(F64)


def softmax_f32(logits, out_bf16=False):
    x = np.asarray(logits, F32)
    e = np.exp(x - x.max(axis=1, keepdims=True)).astype(F32)
    s = np.zeros(x.shape[0], F32)
    for c in range(x.shape[1]):
        s = s + e[:, c]
    p = (e * (F32(1) / s)[:, None]).astype(F32)
    return (to_bf16(p) if out_bf16 else p).astype(F64)
