"""Float64 definitions of the training kernels (include/vc_hip.h, "Training step"; csrc/vc_train.hip and vc_conv_wgrad
of csrc/vc_gemm.hip), plain torch / numpy, one function per exported operation.

  bn_stats            vc_bn_train_stats (vc_hip.h:479-487): batch mean, biased variance, rstd = 1 / sqrt(var + eps),
                      scale = gamma rstd, shift = beta - mean scale, moving = moving decay + new (1 - decay) with the
                      Bessel-corrected variance M / (M - 1) var (M = 1: var)
  bn_stats_f32        the same figures from a float32 two-pass mean-then-variance loop over the rows: what a careful
                      float32 kernel can reach; the device tolerance is a multiple of ITS error against bn_stats
  routing_bits        vc_bn_post_routing (vc_hip.h:498-505): bit 0 a > 0, bit 1 own frame's pool output (last frame of a
                      window or a >= successor), bit 2 previous frame's (t > 0 and a > predecessor), a = relu(x scale + shift)
  routing_close       where one of those comparisons is closer than `margin`: float32 may decide either way there
  bn_backward         vc_bn_backward (vc_hip.h:491-497), modes 0 / 1 / 2, routing bits given
  highway_backward    vc_highway_backward (vc_hip.h:508-511), paired column layout
  transpose_pad       vc_transpose_pad (vc_hip.h:341-347)
  wgrad               vc_conv_wgrad (vc_hip.h:319-339): dW[j Cin + c, o] = sum_m X[m + j + shift0, c] dY[m, o]
  mse_loss            vc_mse_loss (vc_hip.h:533-537)
  softmax_ce          vc_softmax_ce (vc_hip.h:549-554)
  adam                vc_adam_step (vc_hip.h:555-559)
  gru_train           vc_gru_train_forward (vc_hip.h:560-563); differentiable: vc_gru_backward (:564-570) is its autograd
  lstm_train          vc_lstm_train_forward (vc_hip.h:538-544); differentiable: vc_lstm_backward (:545-548)
  affine_act, relu_dropout_backward, axpby, col_sum: vc_hip.h:488-490, 506-507, 516-532, 512-514

Tensors are torch float64 unless said otherwise; activations are [M = N T, C] with T frames per window.
"""
import numpy as np
import torch

F64 = torch.float64


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


def bn_stats(X, gamma, beta, eps, moving_mean=None, moving_var=None, decay=0.999):
    X, gamma, beta = (_t(a).to(F64) for a in (X, gamma, beta))
    M = X.shape[0]
    mean = X.mean(0)
    var = ((X - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    r = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale)
    if moving_mean is not None:
        unb = var * (M / (M - 1.0) if M > 1 else 1.0)
        r['moving_mean'] = _t(moving_mean).to(F64) * decay + mean * (1.0 - decay)
        r['moving_var'] = _t(moving_var).to(F64) * decay + unb * (1.0 - decay)
    return r


def bn_stats_f32(X, gamma, beta, eps, moving_mean=None, moving_var=None, decay=0.999):
    """Every operation rounded to float32: running sum of the rows -> mean, running sum of (x - mean)^2 -> variance."""
    f = np.float32
    X, gamma, beta = (np.asarray(_t(a).numpy(), dtype=f) for a in (X, gamma, beta))
    M = X.shape[0]
    s = np.zeros(X.shape[1], f)
    for r in range(M):
        s = s + X[r]
    mean = s / f(M)
    q = np.zeros(X.shape[1], f)
    for r in range(M):
        d = X[r] - mean
        q = q + d * d
    var = q / f(M)
    rstd = f(1) / np.sqrt(var + f(eps))
    scale = gamma * rstd
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale)
    if moving_mean is not None:
        unb = var * (f(M) / f(M - 1) if M > 1 else f(1))
        out['moving_mean'] = np.asarray(moving_mean, f) * f(decay) + mean * (f(1) - f(decay))
        out['moving_var'] = np.asarray(moving_var, f) * f(decay) + unb * (f(1) - f(decay))
    return {k: torch.from_numpy(np.asarray(v, f)).to(F64) for k, v in out.items()}


def bn_stats_magnitude(X, gamma, beta, eps, moving_mean=None, moving_var=None, decay=0.999):
    """Per channel, the size of the terms each figure is made of: errors are reported relative to these (a mean near zero
    or a shift that cancels has no meaningful relative error of its own)."""
    r = bn_stats(X, gamma, beta, eps, moving_mean, moving_var, decay)
    std = torch.sqrt(r['var'])
    g, b = _t(gamma).to(F64).abs(), _t(beta).to(F64).abs()
    m = dict(mean=r['mean'].abs() + std, rstd=r['rstd'], scale=g * r['rstd'], shift=b + (r['mean'] * r['scale']).abs())
    if moving_mean is not None:
        M = X.shape[0]
        unb = r['var'] * (M / (M - 1.0) if M > 1 else 1.0)
        m['moving_mean'] = _t(moving_mean).to(F64).abs() * decay + (r['mean'].abs() + std) * (1.0 - decay)
        m['moving_var'] = _t(moving_var).to(F64).abs() * decay + unb * (1.0 - decay)
    return m


def _post_act(X, scale, shift, T):
    X = _t(X).to(F64)
    pre = X * _t(scale).to(F64) + _t(shift).to(F64)
    M, C = pre.shape
    return pre.view(M // T, T, C), torch.clamp(pre, min=0.0).view(M // T, T, C)


def routing_bits(X, scale, shift, T):
    pre, a = _post_act(X, scale, shift, T)
    pos = a > 0
    own = torch.ones_like(pos)
    own[:, :-1] = a[:, :-1] >= a[:, 1:]
    prev = torch.zeros_like(pos)
    prev[:, 1:] = a[:, 1:] > a[:, :-1]
    bits = pos.to(torch.uint8) * (1 + 2 * own.to(torch.uint8) + 4 * prev.to(torch.uint8))
    return bits.reshape(X.shape[0], X.shape[1])


def routing_close(X, scale, shift, T, margin=1e-5):
    """True where a float32 evaluation may take another decision than routing_bits: the pre-activation within `margin`
    of zero, or the activation within `margin` of a neighbour it is compared with (elements safely below zero never
    route anything, whatever their neighbours)."""
    pre, a = _post_act(X, scale, shift, T)
    close = pre.abs() < margin
    close[:, :-1] |= (a[:, :-1] - a[:, 1:]).abs() < margin
    close[:, 1:] |= (a[:, 1:] - a[:, :-1]).abs() < margin
    close &= pre > -margin
    return close.reshape(X.shape[0], X.shape[1])


def bn_backward(G, X, T, gamma, mean, rstd, mode, bits=None):
    """-> dX, dgamma, dbeta.  mode 0: G is d/d bn(X); 1: d/d relu(bn(X)); 2: d/d maxpool(relu(bn(X))).  bits [M, C]: the
    routing decisions (routing_bits, or the device's own)."""
    G, X, gamma, mean, rstd = (_t(a).to(F64) for a in (G, X, gamma, mean, rstd))
    M, C = X.shape
    if mode == 0:
        d = G
    else:
        b = _t(bits).to(torch.int64)
        pos, own, prev = ((((b >> k) & 1).to(F64)) for k in range(3))
        if mode == 1:
            d = G * pos
        else:
            G3 = G.view(M // T, T, C)
            Gp = torch.zeros_like(G3)
            Gp[:, 1:] = G3[:, :-1]
            d = pos * (own * G + prev * Gp.reshape(M, C))
    xh = (X - mean) * rstd
    dbeta = d.sum(0)
    dgamma = (d * xh).sum(0)
    dX = gamma * rstd * (d - dbeta / M - xh * dgamma / M)
    return dX, dgamma, dbeta


def paired_columns(H):
    """Columns of unit j's dense1 / dense2 pre-activations in the highway kernels' layout: per 64 columns 32 x dense1 |
    32 x dense2."""
    j = np.arange(H)
    ch = 64 * (j >> 5) + (j & 31)
    return ch, ch + 32


def highway_backward(pre, X, dO, H):
    """pre [M, NP] paired layout -> d_pre [M, NP] (padding columns zero), dX_direct [M, H]."""
    pre, X, dO = (_t(a).to(F64) for a in (pre, X, dO))
    ch, ct = paired_columns(H)
    ph, pt = pre[:, ch], pre[:, ct]
    h, t = torch.clamp(ph, min=0.0), torch.sigmoid(pt)
    dpre = torch.zeros_like(pre)
    dpre[:, ch] = dO * t * (ph > 0).to(F64)
    dpre[:, ct] = dO * (h - X) * t * (1.0 - t)
    return dpre, dO * (1.0 - t)


def transpose_pad(X, T, scale=None, shift=None, relu=False, pool=False, row_shift=0, ldt=None, pad=0):
    """-> XT [C, ldt] float64 with XT[c, pad + m] = pro(X)[m + row_shift, c], zero where the shifted frame leaves its
    window and in both margins; and the same-shaped bound of one float32 rounding of the affine, ulp(|x scale| + |shift|)
    (zero without an affine: the data is then copied exactly)."""
    X = _t(X).to(F64)
    M, C = X.shape
    ldt = M + 2 * pad if ldt is None else ldt
    v = X
    err = torch.zeros_like(X)
    if scale is not None:
        sc, sh = _t(scale).to(F64), _t(shift).to(F64)
        v = X * sc + sh
        err = ((X * sc).abs() + sh.abs()) * 2.0 ** -23
    if relu:
        v = torch.clamp(v, min=0.0)
    if pool:
        v3, e3 = v.view(M // T, T, C).clone(), err.view(M // T, T, C).clone()
        v3[:, :-1] = torch.maximum(v3[:, :-1], v.view(M // T, T, C)[:, 1:])
        e3[:, :-1] = torch.maximum(e3[:, :-1], err.view(M // T, T, C)[:, 1:])
        v, err = v3.reshape(M, C), e3.reshape(M, C)
    t = torch.arange(M) % T
    ok = ((t + row_shift >= 0) & (t + row_shift < T)).to(F64)[:, None]
    src = torch.clamp(torch.arange(M) + row_shift, 0, M - 1)
    out, bound = torch.zeros((C, ldt), dtype=F64), torch.zeros((C, ldt), dtype=F64)
    out[:, pad:pad + M] = (v[src] * ok).t()
    bound[:, pad:pad + M] = (err[src] * ok).t()
    return out, bound


def wgrad(X, dY, T, taps, shift0):
    """Filter gradient in TF layout [taps * Cin, N]; a frame of another window contributes nothing."""
    X, dY = _t(X).to(F64), _t(dY).to(F64)
    M, Cin = X.shape
    t = torch.arange(M) % T
    rows = []
    for j in range(taps):
        s = j + shift0
        ok = ((t + s >= 0) & (t + s < T)).to(F64)[:, None]
        Xs = X[torch.clamp(torch.arange(M) + s, 0, M - 1)] * ok
        rows.append(Xs.t() @ dY)
    return torch.cat(rows, 0)


def mse_loss(y, t, weight):
    """-> loss = weight mean((y - t)^2), dY = 2 weight / n (y - t)."""
    y, t = _t(y).to(F64), _t(t).to(F64)
    d = y - t
    return weight * (d * d).mean(), 2.0 * weight / d.numel() * d


def softmax_ce(logits, target):
    """-> [mean cross-entropy with float labels, accuracy of argmax vs argmax (first maximum), mean squared error of the
    posteriors], dlogits = (softmax sum(target) - target) / M."""
    x, t = _t(logits).to(F64), _t(target).to(F64)
    M = x.shape[0]
    logp = x - torch.logsumexp(x, 1, keepdim=True)
    p = torch.exp(logp)
    first = lambda a: torch.from_numpy(np.argmax(a.numpy(), axis=1))       # numpy: the first maximum
    out3 = torch.stack([-(t * logp).sum(1).mean(), (first(x) == first(t)).to(F64).mean(), ((p - t) ** 2).mean()])
    return out3, (p * t.sum(1, keepdim=True) - t) / M


def adam(p, g, m, v, lr_t, beta1, beta2, epsilon, grad_scale):
    p, g, m, v = (_t(a).to(F64) for a in (p, g, m, v))
    g = g * grad_scale
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return p - lr_t * m / (torch.sqrt(v) + epsilon), m, v


def gru_train(xproj, wh, N, T, H):
    """tf.contrib.rnn.GRUCell under bidirectional_dynamic_rnn with the input projections given: xproj [N T, 6H] (per
    direction r | u | c), wh[d] [H, 3H].  r, u = sigmoid(x + h Wg); c = tanh(x + (r h) Wc); h' = u h + (1 - u) c; the
    backward direction runs t = T-1 .. 0.  -> out [N T, 2H], gates [2, N T, 3H] (r | u | c), rh [2, N T, H].
    Differentiable w.r.t. xproj."""
    outs, gates, rhs = [], [], []
    for d in range(2):
        x3 = xproj.view(N, T, 6 * H)[:, :, d * 3 * H:(d + 1) * 3 * H]
        h = torch.zeros((N, H), dtype=xproj.dtype)
        hs, gs, rs = [None] * T, [None] * T, [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            g = torch.sigmoid(x3[:, t, :2 * H] + h @ wh[d][:, :2 * H])
            r, u = g[:, :H], g[:, H:]
            c = torch.tanh(x3[:, t, 2 * H:] + (r * h) @ wh[d][:, 2 * H:])
            rs[t] = r * h
            h = u * h + (1 - u) * c
            hs[t], gs[t] = h, torch.cat([g, c], 1)
        outs.append(torch.stack(hs, 1))
        gates.append(torch.stack(gs, 1).reshape(N * T, 3 * H))
        rhs.append(torch.stack(rs, 1).reshape(N * T, H))
    return torch.cat(outs, 2).reshape(N * T, 2 * H), torch.stack(gates), torch.stack(rhs)


def lstm_train(xproj, wh, N, T, H):
    """tf.contrib.rnn.LSTMCell (forget_bias 1.0, gate order i, j, f, o) under bidirectional_dynamic_rnn: xproj [N T, 8H],
    wh[d] [H, 4H].  c' = c sig(f + 1) + sig(i) tanh(j); h' = tanh(c') sig(o).  -> out [N T, 2H], the ACTIVATED gates
    [2, N T, 4H], the cell states [2, N T, H].  Differentiable w.r.t. xproj."""
    outs, gates, cs = [], [], []
    for d in range(2):
        x3 = xproj.view(N, T, 8 * H)[:, :, d * 4 * H:(d + 1) * 4 * H]
        h = torch.zeros((N, H), dtype=xproj.dtype)
        c = torch.zeros((N, H), dtype=xproj.dtype)
        hs, gs, cc = [None] * T, [None] * T, [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            z = x3[:, t] + h @ wh[d]
            gi, gj = torch.sigmoid(z[:, :H]), torch.tanh(z[:, H:2 * H])
            gf, go = torch.sigmoid(z[:, 2 * H:3 * H] + 1.0), torch.sigmoid(z[:, 3 * H:])
            c = c * gf + gi * gj
            h = torch.tanh(c) * go
            hs[t], gs[t], cc[t] = h, torch.cat([gi, gj, gf, go], 1), c
        outs.append(torch.stack(hs, 1))
        gates.append(torch.stack(gs, 1).reshape(N * T, 4 * H))
        cs.append(torch.stack(cc, 1).reshape(N * T, H))
    return torch.cat(outs, 2).reshape(N * T, 2 * H), torch.stack(gates), torch.stack(cs)


def affine_act(X, scale, shift, relu, R):
    v = _t(X).to(F64)
    if scale is not None:
        v = v * _t(scale).to(F64)
    if shift is not None:
        v = v + _t(shift).to(F64)
    if relu:
        v = torch.clamp(v, min=0.0)
    return v if R is None else v + _t(R).to(F64)


def relu_dropout_backward(dY, Y, inv_keep):
    return torch.where(_t(Y) > 0, _t(dY).to(F64) * inv_keep, torch.zeros((), dtype=F64))


def axpby(a, X, b, Y):
    return a * _t(X).to(F64) + b * _t(Y).to(F64)


def col_sum(X):
    """-> column sums and the column sums of magnitudes (what a float32 reduction's error is measured against)."""
    X = _t(X).to(F64)
    return X.sum(0), X.abs().sum(0)
