"""tests/train_kernels_ref.py checked without a GPU: every float64 definition the device tests compare the training
kernels with, against float64 torch.autograd of the obvious composition of torch's own operators.  Inputs are continuous
draws (no ties), so max-pool / relu / argmax routing is unambiguous on both sides."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_kernels_ref as R

F64 = torch.float64
TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = torch.as_tensor(a).to(F64), torch.as_tensor(b).to(F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    e = float((a - b).abs().max() / max(1.0, float(b.abs().max())))
    assert e < tol, e


def _post(y, mode, N, T):
    """bn output [M, C] -> what vc_bn_backward's upstream gradient is taken of: relu, then max_pooling1d(2, 1, 'same')
    (TensorFlow pads on the right: the last frame of a window keeps its value)."""
    if mode == 0:
        return y
    a = torch.relu(y)
    if mode == 1:
        return a
    C = y.shape[1]
    a3 = a.view(N, T, C).permute(0, 2, 1)
    p = F.max_pool1d(F.pad(a3, (0, 1), value=float('-inf')), 2, 1)
    return p.permute(0, 2, 1).reshape(N * T, C)


@pytest.mark.parametrize('M', [1, 7, 200])
def test_bn_stats_match_torch_batch_norm(M):
    rng = np.random.RandomState(M)
    C, eps, decay = 5, 1e-3, 0.9
    X = torch.from_numpy(rng.standard_normal((M, C)) * 0.7 + 3.0)
    gamma, beta = torch.from_numpy(rng.uniform(0.5, 1.5, C)), torch.from_numpy(rng.standard_normal(C))
    mm, mv = torch.from_numpy(rng.standard_normal(C)), torch.from_numpy(rng.uniform(0.5, 2.0, C))
    r = R.bn_stats(X, gamma, beta, eps, mm, mv, decay)
    if M > 1:
        rm, rv = mm.clone(), mv.clone()
        y = F.batch_norm(X, rm, rv, gamma, beta, training=True, momentum=1.0 - decay, eps=eps)
        _close(X * r['scale'] + r['shift'], y)
        _close(r['moving_mean'], rm)
        _close(r['moving_var'], rv)
    else:
        _close(r['mean'], X[0])
        _close(r['var'], torch.zeros(C, dtype=F64))
        _close(r['moving_var'], mv * decay)
    _close(r['rstd'], 1.0 / torch.sqrt(X.var(0, unbiased=False) + eps))
    # the float32 two-pass restatement computes the same figures, to float32 accuracy, offset mean included
    Xo = X * 0.05 + 12.8                       # |mean| = 256 sigma
    r64, r32 = R.bn_stats(Xo, gamma, beta, eps, mm, mv, decay), R.bn_stats_f32(Xo, gamma, beta, eps, mm, mv, decay)
    mag = R.bn_stats_magnitude(Xo, gamma, beta, eps, mm, mv, decay)
    for k in mag:
        assert float(((r32[k] - r64[k]).abs() / mag[k]).max()) < 3e-6, k


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('N,T', [(3, 1), (5, 4), (2, 50)])
def test_bn_backward_matches_autograd(mode, N, T):
    rng = np.random.RandomState(10 * N + T + mode)
    M, C, eps = N * T, 6, 1e-3
    X = torch.from_numpy(rng.standard_normal((M, C))).requires_grad_(True)
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, C)).requires_grad_(True)
    beta = torch.from_numpy(rng.standard_normal(C) * 0.3).requires_grad_(True)
    G = torch.from_numpy(rng.standard_normal((M, C)))
    if M > 1:
        y = F.batch_norm(X, None, None, gamma, beta, training=True, eps=eps)
    else:
        y = (X - X.mean(0)) / torch.sqrt(X.var(0, unbiased=False) + eps) * gamma + beta
    (_post(y, mode, N, T) * G).sum().backward()
    st = R.bn_stats(X.detach(), gamma.detach(), beta.detach(), eps)
    bits = R.routing_bits(X.detach(), st['scale'], st['shift'], T)
    dX, dgamma, dbeta = R.bn_backward(G, X.detach(), T, gamma.detach(), st['mean'], st['rstd'], mode, bits)
    _close(dX, X.grad)
    _close(dgamma, gamma.grad)
    _close(dbeta, beta.grad)


def test_routing_bits_follow_the_tie_rule_on_a_grid():
    """Integer activations (scale 1, shift 0), one window of 6 frames and one of 1: own frame on >=, previous frame on
    strict >, nothing through a zero activation, a window's last frame never looks past it."""
    x = torch.tensor([[2.0], [2.0], [1.0], [0.0], [-1.0], [3.0]], dtype=F64)
    one, zero = torch.ones(1, dtype=F64), torch.zeros(1, dtype=F64)
    assert R.routing_bits(x, one, zero, 6)[:, 0].tolist() == [3, 3, 3, 0, 0, 7]
    # as windows of 3: frame 2 is a last frame (own), frame 3 is a first frame (no previous)
    assert R.routing_bits(x, one, zero, 3)[:, 0].tolist() == [3, 3, 3, 0, 0, 7]
    assert R.routing_bits(x, one, zero, 1)[:, 0].tolist() == [3, 3, 3, 0, 0, 3]
    assert R.routing_bits(torch.tensor([[1.0], [2.0], [5.0], [4.0]], dtype=F64), one, zero, 2)[:, 0].tolist() == [1, 7, 3, 3]


def routing_inputs(M, C, ld, seed):
    """The random inputs of the device routing test (tests/test_train_kernels_gpu.py): unit-variance activations, scales
    around 1: neighbouring activations differ by O(1), so a fraction of about 1e-5 / 1 of them is within 1e-5."""
    rng = np.random.RandomState(seed)
    X = np.full((M, ld), np.nan, np.float32)
    X[:, :C] = rng.standard_normal((M, C))
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    shift = (rng.standard_normal(C) * 0.3).astype(np.float32)
    return X, scale, shift


ROUTING_SHAPES = [(50, 1, 257, 300), (13, 4, 33, 40), (8, 50, 1, 2), (5, 64, 33, 33 + 7), (3, 64, 257, 260), (100, 1, 33, 64),
                  (50, 4, 1, 8)]            # N, T, C, ld


@pytest.mark.parametrize('N,T,C,ld', ROUTING_SHAPES)
def test_routing_exclusion_cap_met_by_the_reference_alone(N, T, C, ld):
    X, scale, shift = routing_inputs(N * T, C, ld, N + T + C)
    close = R.routing_close(torch.from_numpy(X[:, :C]), torch.from_numpy(scale), torch.from_numpy(shift), T)
    assert float(close.to(F64).mean()) <= 0.01


@pytest.mark.parametrize('H', [32, 40, 72])
def test_highway_backward_matches_autograd(H):
    rng = np.random.RandomState(H)
    M, NP = 9, 64 * ((H + 31) // 32)
    ch, ct = R.paired_columns(H)
    assert len(set(ch) | set(ct)) == 2 * H and max(ct) < NP
    pre = torch.from_numpy(rng.standard_normal((M, NP))).requires_grad_(True)
    X = torch.from_numpy(rng.standard_normal((M, H))).requires_grad_(True)
    dO = torch.from_numpy(rng.standard_normal((M, H)))
    t = torch.sigmoid(pre[:, ct])
    out = torch.relu(pre[:, ch]) * t + X * (1.0 - t)
    (out * dO).sum().backward()
    dpre, dXd = R.highway_backward(pre.detach(), X.detach(), dO, H)
    _close(dpre, pre.grad)
    _close(dXd, X.grad)


@pytest.mark.parametrize('row_shift', [-5, -1, 0, 1, 4])
@pytest.mark.parametrize('affine,relu,pool', [(0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 0, 1)])
def test_transpose_pad_matches_composition(row_shift, affine, relu, pool):
    rng = np.random.RandomState(3)
    N, T, C, pad, ldt = 4, 5, 7, 3, 30
    X = torch.from_numpy(rng.standard_normal((N * T, C)))
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, C)) if affine else None
    sh = torch.from_numpy(rng.standard_normal(C)) if affine else None
    got, _ = R.transpose_pad(X, T, sc, sh, relu, pool, row_shift, ldt, pad)
    v = X * sc + sh if affine else X
    v = _post(v, 2 if relu else 0, N, T) if (relu and pool) else (torch.relu(v) if relu else v)
    if pool and not relu:
        v3 = v.view(N, T, C).permute(0, 2, 1)
        v = F.max_pool1d(F.pad(v3, (0, 1), value=float('-inf')), 2, 1).permute(0, 2, 1).reshape(N * T, C)
    v3 = v.view(N, T, C)
    sh3 = torch.zeros_like(v3)
    for t in range(T):
        if 0 <= t + row_shift < T:
            sh3[:, t] = v3[:, t + row_shift]
    want = torch.zeros((C, ldt), dtype=F64)
    want[:, pad:pad + N * T] = sh3.reshape(N * T, C).t()
    _close(got, want)


@pytest.mark.parametrize('taps,T', [(1, 4), (2, 4), (3, 8), (5, 4), (8, 8)])
def test_wgrad_matches_conv1d_autograd(taps, T):
    rng = np.random.RandomState(taps)
    N, Cin, Cout = 3, 5, 4
    pad_l = taps // 2
    X = torch.from_numpy(rng.standard_normal((N * T, Cin)))
    dY = torch.from_numpy(rng.standard_normal((N * T, Cout)))
    W = torch.from_numpy(rng.standard_normal((Cout, Cin, taps))).requires_grad_(True)
    x3 = F.pad(X.view(N, T, Cin).permute(0, 2, 1), (pad_l, taps - 1 - pad_l))
    y = F.conv1d(x3, W).permute(0, 2, 1).reshape(N * T, Cout)
    (y * dY).sum().backward()
    want = W.grad.permute(2, 1, 0).reshape(taps * Cin, Cout)                 # TF layout [taps, Cin, Cout]
    _close(R.wgrad(X, dY, T, taps, -pad_l), want)


def test_mse_loss_matches_autograd():
    rng = np.random.RandomState(1)
    y = torch.from_numpy(rng.standard_normal((11, 7))).requires_grad_(True)
    t = torch.from_numpy(rng.standard_normal((11, 7)))
    (400.0 * F.mse_loss(y, t)).backward()
    loss, dY = R.mse_loss(y.detach(), t, 400.0)
    _close(loss, 400.0 * F.mse_loss(y.detach(), t))
    _close(dY, y.grad)


@pytest.mark.parametrize('normalised', [True, False])
def test_softmax_ce_matches_autograd(normalised):
    rng = np.random.RandomState(2)
    M, C = 9, 13
    x = torch.from_numpy(rng.standard_normal((M, C)) * 3).requires_grad_(True)
    t = torch.from_numpy(rng.uniform(0.0, 1.0, (M, C)))
    if normalised:
        t = t / t.sum(1, keepdim=True)
    F.cross_entropy(x, t).backward()
    out3, dl = R.softmax_ce(x.detach(), t)
    _close(out3[0], F.cross_entropy(x.detach(), t))
    _close(out3[1], (x.detach().argmax(1) == t.argmax(1)).to(F64).mean())
    _close(out3[2], F.mse_loss(torch.softmax(x.detach(), 1), t))
    _close(dl, x.grad)
    # exact ties: the first maximum wins on both sides
    xt = torch.tensor([[1.0, 5.0, 5.0], [5.0, 1.0, 5.0]], dtype=F64)
    tt = torch.tensor([[0.0, 0.5, 0.5], [0.2, 0.4, 0.4]], dtype=F64)
    assert float(R.softmax_ce(xt, tt)[0][1]) == 0.5


def test_adam_matches_torch_adam():
    """torch's Adam divides by sqrt(v) / sqrt(1 - b2^t) + eps; the TensorFlow form by sqrt(v) + eps with the correction
    in lr_t: equal when torch is given eps / sqrt(1 - b2^t).  Three steps, so m and v are non-zero from the second."""
    rng = np.random.RandomState(5)
    lr, b1, b2, eps = 1e-2, 0.9, 0.99, 1e-6
    p0 = torch.from_numpy(rng.standard_normal(20))
    p, m, v = p0.clone(), torch.zeros(20, dtype=F64), torch.zeros(20, dtype=F64)
    for t in range(1, 4):
        g = torch.from_numpy(rng.standard_normal(20))
        q = torch.nn.Parameter(p.clone())
        opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps / np.sqrt(1 - b2 ** t))
        if t > 1:
            opt.state[q] = {'step': torch.tensor(float(t - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
        q.grad = 0.5 * g
        opt.step()
        p, m, v = R.adam(p, g, m, v, lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t), b1, b2, eps, 0.5)
        _close(p, q.detach(), 1e-10)
        _close(m, opt.state[q]['exp_avg'])
        _close(v, opt.state[q]['exp_avg_sq'])


def _gru_loop(xp, wh, N, T, H):
    """The cell written out per window and step in numpy (no batching, no autograd)."""
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    out, gates, rh = np.zeros((N * T, 2 * H)), np.zeros((2, N * T, 3 * H)), np.zeros((2, N * T, H))
    for d in range(2):
        for n in range(N):
            h = np.zeros(H)
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                x = xp[n * T + t, d * 3 * H:(d + 1) * 3 * H]
                g = sig(x[:2 * H] + h @ wh[d][:, :2 * H])
                r, u = g[:H], g[H:]
                c = np.tanh(x[2 * H:] + (r * h) @ wh[d][:, 2 * H:])
                rh[d, n * T + t] = r * h
                h = u * h + (1 - u) * c
                out[n * T + t, d * H:(d + 1) * H] = h
                gates[d, n * T + t] = np.concatenate([g, c])
    return out, gates, rh


def test_gru_train_matches_loop_and_finite_differences():
    rng = np.random.RandomState(7)
    N, T, H = 2, 3, 4
    xp = torch.from_numpy(rng.standard_normal((N * T, 6 * H)))
    wh = [torch.from_numpy(rng.standard_normal((H, 3 * H)) * 0.5) for _ in range(2)]
    out, gates, rh = R.gru_train(xp, wh, N, T, H)
    o2, g2, r2 = _gru_loop(xp.numpy(), [w.numpy() for w in wh], N, T, H)
    _close(out, o2)
    _close(gates, g2)
    _close(rh, r2)
    assert torch.autograd.gradcheck(lambda x: R.gru_train(x, wh, N, T, H)[0], (xp.clone().requires_grad_(True),))


def test_lstm_train_matches_torch_lstm_cell():
    """torch's LSTM cell (gate order i, f, g, o, no forget bias) fed the given projections through an identity input
    weight and the forget bias 1.0 as its recurrent bias."""
    rng = np.random.RandomState(8)
    N, T, H = 3, 4, 5
    xp = torch.from_numpy(rng.standard_normal((N * T, 8 * H))).requires_grad_(True)
    wh = [torch.from_numpy(rng.standard_normal((H, 4 * H)) * 0.5) for _ in range(2)]
    dG = torch.from_numpy(rng.standard_normal((N * T, 2 * H)))
    out, gates, cst = R.lstm_train(xp, wh, N, T, H)
    (out * dG).sum().backward()
    order = np.concatenate([np.arange(H), 2 * H + np.arange(H), H + np.arange(H), 3 * H + np.arange(H)])   # i f j o
    xq = xp.detach().clone().requires_grad_(True)
    b_hh = torch.zeros(4 * H, dtype=F64)
    b_hh[H:2 * H] = 1.0
    outs = []
    for d in range(2):
        x3 = xq.view(N, T, 8 * H)[:, :, d * 4 * H:(d + 1) * 4 * H][:, :, order]
        h, c = torch.zeros((N, H), dtype=F64), torch.zeros((N, H), dtype=F64)
        hs = [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            h, c = torch._VF.lstm_cell(x3[:, t], (h, c), torch.eye(4 * H, dtype=F64), wh[d][:, order].t().contiguous(),
                                       torch.zeros(4 * H, dtype=F64), b_hh)
            hs[t] = h
            _close(cst[d].view(N, T, H)[:, t].detach(), c.detach())
        outs.append(torch.stack(hs, 1))
    want = torch.cat(outs, 2).reshape(N * T, 2 * H)
    (want * dG).sum().backward()
    _close(out.detach(), want.detach())
    _close(xp.grad, xq.grad)
    # the saved gates are the activated ones, forget bias included
    z0 = xp.detach().view(N, T, 8 * H)[:, 0, :4 * H]
    g0 = gates[0].view(N, T, 4 * H)[:, 0].detach()
    _close(g0, torch.cat([torch.sigmoid(z0[:, :H]), torch.tanh(z0[:, H:2 * H]), torch.sigmoid(z0[:, 2 * H:3 * H] + 1.0),
                          torch.sigmoid(z0[:, 3 * H:])], 1))


def test_elementwise_references():
    rng = np.random.RandomState(9)
    X, Y = torch.from_numpy(rng.standard_normal((6, 5))), torch.from_numpy(rng.standard_normal((6, 5)))
    sc, sh = torch.from_numpy(rng.standard_normal(5)), torch.from_numpy(rng.standard_normal(5))
    _close(R.affine_act(X, sc, sh, True, Y), torch.relu(X * sc + sh) + Y)
    _close(R.affine_act(X, None, None, False, None), X)
    _close(R.axpby(0.3, X, -2.0, Y), 0.3 * X - 2.0 * Y)
    z = X.clone().requires_grad_(True)
    mask = torch.from_numpy((rng.uniform(size=(6, 5)) < 0.8).astype(np.float64)) / 0.8
    y = torch.relu(z) * mask
    (y * Y).sum().backward()
    _close(R.relu_dropout_backward(Y * (mask > 0), y.detach(), 1.0 / 0.8), z.grad)
    s, a = R.col_sum(X)
    _close(s, X.sum(0))
    _close(a, X.abs().sum(0))
