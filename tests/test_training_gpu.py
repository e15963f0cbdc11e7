"""Decoder training step on the MI355X (float32) against autograd on the float64 oracle
(oracle/model_oracle.py: TF-1.9 semantics incl. train-mode batch norm, dropout with explicit
masks, weighted MSE, TF-style Adam).  The dropout masks the kernels use are reproduced on the
host from the same stateless hash (splitmix64 of the output element index and the seed,
csrc/vc_gemm.hip: drop_keep_elem) and handed to the oracle, so the comparison is exact in
expectation AND per element.  Tolerance: 2e-3 of each tensor's max |gradient| (float32 MFMA sums
over up to 12,800 frames vs float64), 1e-5 on losses."""
import json

import numpy as np
import pytest
import torch

from conv_gemm_ref import drop_mask as _mask      # host twin of drop_keep_elem (csrc/vc_gemm.hip)
from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu


def _cfg(T=40, dropout=0.1, loss_type='sum'):
    return {'model_name': 'decoder', 'input_shape': [T, 61], 'dropout_rate': dropout, 'is_training': True,
            'use_Cudnn': False, 'use_lstm': False, 'use_target_mel_step2': False,
            'mel_loss_weight': 400, 'stft_loss_weight': 400, 'loss_type': loss_type,
            'learning_rate': 1e-3, 'decay': 1e-3, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8,
            'dropout_seed': 77, 'batch_size': 4,
            'steps_v': [{'embed_size': 64, 'num_conv_banks': 5, 'num_highwaynet_blocks': 2, 'n_output': 80},
                        {'embed_size': 96, 'num_conv_banks': 4, 'num_highwaynet_blocks': 1, 'n_output': 201}]}


def _setup(cfg, N=4, seed=3):
    from decoder import decoder_specs
    T = cfg['input_shape'][0]
    dec = decoder_specs(cfg, None, None)
    w = mo.init_weights(cfg, 'decoder', seed=5, perturb_bn=True)
    dec.store.load_dict(w)
    rng = np.random.RandomState(seed)
    ppg = torch.softmax(torch.from_numpy(rng.standard_normal((N, T, 61)) * 2), -1).float().numpy()
    t_mel = rng.uniform(0, 0.8, (N, T, 80)).astype(np.float32)
    t_stft = rng.uniform(0, 0.8, (N, T, 201)).astype(np.float32)
    return dec, w, ppg, t_mel, t_stft


def _device_routing(tr):
    """The trainer's exported relu / pool routing (training.py export_routing: what its backward pass decided) in the
    oracle's form: per stage the prenet's two relus, the filter bank's relu + max-pool, the first projection's relu and
    every highway block's relu."""
    out = {}
    for k, v in tr.routing.items():
        f64 = lambda t: t.cpu().to(torch.float64)
        out[k.split('/')[-1]] = {'banks': mo.routing_from_bits(v['banks'].cpu()), 'conv1d_1': f64(v['conv1d_1']),
                                 'prenet': tuple(f64(t) for t in v['prenet']),
                                 'highway': None if any(h is None for h in v['highway']) else [f64(h) for h in v['highway']]}
    return out


def _oracle_step(cfg, w, ppg, t_mel, t_stft, seed_base, taps=None, f_mel_pred=None, routing=None):
    N, T = ppg.shape[:2]
    M = N * T
    keep = 1.0 - cfg['dropout_rate']
    masks = {}
    for i, sd in enumerate(cfg['steps_v']):
        E = sd['embed_size']
        sb = seed_base + (0 if i == 0 else 10)
        if keep < 1.0:
            masks['step%d' % (i + 1)] = (torch.from_numpy(_mask(M, E, E, sb + 1, keep)).view(N, T, E),
                                         torch.from_numpy(_mask(M, E // 2, E // 2, sb + 2, keep)).view(N, T, E // 2))
        else:
            masks = None
    wt = mo.to_torch(w, torch.float64, requires_grad=True)
    stats = {}
    ym, ys = mo.decoder_forward(torch.from_numpy(ppg).double(), wt, cfg, is_training=True, masks=masks, stats_out=stats,
                                taps=taps, target_mel=torch.from_numpy(t_mel).double(), f_mel_pred=f_mel_pred,
                                routing=routing)
    ml, sl, loss = mo.decoder_loss(ym, ys, torch.from_numpy(t_mel).double(), torch.from_numpy(t_stft).double(), cfg)
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in wt.items() if v.requires_grad}
    return float(ml.detach()), float(sl.detach()), grads, stats, ym.detach().numpy(), ys.detach().numpy()


@pytest.mark.parametrize('dropout,loss_type', [(0.1, 'sum'), (0.0, 'log')])
def test_train_step_gradients_match_autograd(dropout, loss_type):
    cfg = _cfg(dropout=dropout, loss_type=loss_type)
    dec, w, ppg, t_mel, t_stft = _setup(cfg)
    tr = dec._get_trainer()
    x = torch.from_numpy(ppg).cuda()
    losses = tr.forward_backward(x, torch.from_numpy(t_mel).cuda(), torch.from_numpy(t_stft).cuda())
    ml, sl, grads, stats, ym, ys = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed + 1000 * tr.step_count)
    got = losses.cpu().numpy()
    assert abs(got[0] - ml) < 1e-5 * max(1, ml) and abs(got[1] - sl) < 1e-5 * max(1, sl), (got, ml, sl)
    assert np.abs(tr.y_mel.cpu().numpy().reshape(ym.shape) - ym).max() < 1e-4
    assert np.abs(tr.y_stft.cpu().numpy().reshape(ys.shape) - ys).max() < 1e-4
    assert set(grads) == set(tr.names)
    worst = ('', 0.0)
    for n in tr.names:
        g = tr.g(n).cpu().numpy().astype(np.float64)
        ref = grads[n]
        assert g.shape == ref.shape, n
        err = np.abs(g - ref).max() / max(np.abs(ref).max(), 1e-6)
        if err > worst[1]:
            worst = (n, err)
    assert worst[1] < 2e-3, 'worst gradient mismatch %s: %.3e' % worst
    # moving statistics were updated in place with the Bessel-corrected batch variance
    for n, v in stats.items():
        assert np.abs(dec.store.vars[n].cpu().numpy() - v.numpy()).max() < 1e-5, n


def test_train_step_on_the_split_float16_path_at_a_small_configuration():
    """The same step with stage widths that put the filter bank and the first projection on the split-float16 path at
    shapes far from the shipped ones (training._g16_plan: any H % 64 == 0 with an even K): stage 1 E = 128 -> H = 64 (bank
    forward and the projection's data gradient only), stage 2 E = 256 -> H = 128 (all four forms, 128-column filters as
    single-filter pairs), 4 and 6 banks, 160 frames in 4 windows of 40 (less than one 256-row tile; the filter
    gradients stay on wgrad_kernel: the frame count is not a multiple of 64).  Against autograd on the f64 oracle with
    the device's own relu / pool routing (see test_hp_size_train_step_matches_autograd: at 160 frames ONE relu decided
    the other way moves a bias gradient by several per cent), every gradient element within 1e-4."""
    cfg = _cfg(dropout=0.1)
    cfg['steps_v'][0].update(embed_size=128, num_conv_banks=4)
    cfg['steps_v'][1].update(embed_size=256, num_conv_banks=6)
    dec, w, ppg, t_mel, t_stft = _setup(cfg)
    tr = dec._get_trainer()
    tr.export_routing = True
    x = torch.from_numpy(ppg).cuda()
    losses = tr.forward_backward(x, torch.from_numpy(t_mel).cuda(), torch.from_numpy(t_stft).cuda())
    assert set(tr._g16) == {'decoder/step1', 'decoder/step2'}
    assert 'bank_dgrad' not in tr._g16['decoder/step1'] and 'bank_dgrad' in tr._g16['decoder/step2']
    routing = _device_routing(tr)
    tr.export_routing = False
    ml, sl, grads, stats, ym, ys = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed + 1000 * tr.step_count, routing=routing)
    got = losses.cpu().numpy()
    assert abs(got[0] - ml) < 1e-5 * max(1, ml) and abs(got[1] - sl) < 1e-5 * max(1, sl), (got, ml, sl)
    assert np.abs(tr.y_mel.cpu().numpy().reshape(ym.shape) - ym).max() < 1e-4
    assert np.abs(tr.y_stft.cpu().numpy().reshape(ys.shape) - ys).max() < 1e-4
    worst = ('', 0.0)
    for n in tr.names:
        g = tr.g(n).cpu().numpy().astype(np.float64)
        err = np.abs(g - grads[n]).max() / max(np.abs(grads[n]).max(), 1e-6)
        if err > worst[1]:
            worst = (n, err)
    print('worst gradient mismatch %s %.3e' % worst)
    assert worst[1] < 1e-4, 'worst gradient mismatch %s: %.3e' % worst
    # a second step after Adam: the float16 weight copies were rewritten behind the update (their own stream), the
    # forward pass waits for them -- the loss must move like the float32-MFMA path's does
    tr.apply_gradients(1)
    l2 = tr.forward_backward(x, torch.from_numpy(t_mel).cuda(), torch.from_numpy(t_stft).cuda()).cpu().numpy()
    cfg32 = dict(cfg, train_f16x3=False)
    dec32, _, _, _, _ = _setup(cfg32)
    tr32 = dec32._get_trainer()
    tr32.forward_backward(x, torch.from_numpy(t_mel).cuda(), torch.from_numpy(t_stft).cuda())
    tr32.apply_gradients(1)
    l32 = tr32.forward_backward(x, torch.from_numpy(t_mel).cuda(), torch.from_numpy(t_stft).cuda()).cpu().numpy()
    assert not tr32._g16
    assert np.abs(l2 - l32).max() < 2e-4 * np.abs(l32).max(), (l2, l32)


def test_teacher_forced_stage2_matches_autograd(tmp_path):
    """use_target_mel_step2 (/root/reference/decoder.py:148-152, 258-260, 435-437): stage 2 is fed
    f_mel_pred * y_mel + (1 - f_mel_pred) * target_mel; f_mel_pred is a saved, non-trainable scalar raised per epoch
    as min(1, 1.02 tanh(epoch / target_mel_step2_val)).  Training forward / backward against autograd on the oracle at
    f = 0.3 (the gradient reaches y_mel through the blend with weight f), the inference graph through
    exec_calc_metrics, the schedule, the checkpoint variable."""
    import tf_bundle
    from decoder import decoder_specs
    cfg = _cfg()
    cfg.update(use_target_mel_step2=True, target_mel_step2_val=500, model_path=str(tmp_path))
    dec = decoder_specs(cfg, None, None)
    fname = 'decoder/step2/inputs_step2/f_mel_pred_tf'
    assert fname in dec.store.vars and fname not in dec.store.trainable_names('decoder/')
    w = mo.init_weights(cfg, 'decoder', seed=5, perturb_bn=True)
    dec.store.load_dict(w, strict=False)
    rng = np.random.RandomState(3)
    ppg = torch.softmax(torch.from_numpy(rng.standard_normal((4, 40, 61)) * 2), -1).float().numpy()
    t_mel = rng.uniform(0, 0.8, (4, 40, 80)).astype(np.float32)
    t_stft = rng.uniform(0, 0.8, (4, 40, 201)).astype(np.float32)
    dec._set_f_mel_pred(0.3)
    tr = dec._get_trainer()
    losses = tr.forward_backward(*(torch.from_numpy(a).cuda() for a in (ppg, t_mel, t_stft))).cpu().numpy()
    ml, sl, grads, stats, ym, ys = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed, f_mel_pred=0.3)
    assert abs(losses[0] - ml) < 1e-5 * max(1, ml) and abs(losses[1] - sl) < 1e-5 * max(1, sl), (losses, ml, sl)
    assert np.abs(tr.y_stft.cpu().numpy().reshape(ys.shape) - ys).max() < 1e-4
    worst = ('', 0.0)
    for n in tr.names:
        err = np.abs(tr.g(n).cpu().numpy() - grads[n]).max() / max(np.abs(grads[n]).max(), 1e-6)
        if err > worst[1]:
            worst = (n, err)
    assert worst[1] < 2e-3, 'worst gradient mismatch %s: %.3e' % worst
    # f = 0: stage 1 gets no gradient from the stft loss at all (its input is the target alone)
    dec._set_f_mel_pred(0.0)
    tr.forward_backward(*(torch.from_numpy(a).cuda() for a in (ppg, t_mel, t_stft)))
    _, _, g0, _, _, _ = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed, f_mel_pred=0.0)
    n1 = 'decoder/step1/y_logits/kernel'
    assert np.abs(tr.g(n1).cpu().numpy() - g0[n1]).max() < 2e-3 * np.abs(g0[n1]).max()
    # the schedule (float32 ops of the graph) and the checkpoint
    dec.opt_state['dec_opt/epoch'] = np.int32(250)
    f = dec._f_mel_pred_update()
    assert abs(f - min(1.0, 1.02 * np.tanh(250 / 500.0))) < 1e-6 and abs(float(dec.store.vars[fname]) - f) < 1e-7
    dec.opt_state['dec_opt/epoch'] = np.int32(5000)
    assert dec._f_mel_pred_update() == 1.0
    dec._set_f_mel_pred(0.3)
    dec.save(verbose=False)
    ck = tf_bundle.read_bundle(tf_bundle.latest_checkpoint(str(tmp_path)))
    assert abs(float(ck[fname]) - 0.3) < 1e-7
    # inference graph of the same configuration: needs target_mel (like the reference's placeholder), predict refuses
    icfg = dict(cfg, is_training=False)
    idec = decoder_specs(icfg, None, None)
    idec.restore()
    assert abs(idec.f_mel_pred - 0.3) < 1e-7
    got = idec.exec_calc_metrics(ppg, t_mel, t_stft)
    wi = {k: v for k, v in ck.items() if k in w}
    ym_i, ys_i = mo.decoder_forward(torch.from_numpy(ppg).double(), mo.to_torch(wi, torch.float64), icfg,
                                    target_mel=torch.from_numpy(t_mel).double(), f_mel_pred=0.3)
    mli, sli, _ = mo.decoder_loss(ym_i, ys_i, torch.from_numpy(t_mel).double(), torch.from_numpy(t_stft).double(), icfg)
    assert abs(got[0] - float(mli)) < 1e-4 * max(1, float(mli)) and abs(got[1] - float(sli)) < 1e-4 * max(1, float(sli))
    with pytest.raises(Exception, match='use_target_mel_step2'):
        idec.predict(ppg)


def test_lstm_stage_train_step_matches_autograd(tmp_path):
    """use_lstm in training (/root/reference/modules.py:207-243, 347-350 under tf.gradients; no shipped configuration
    sets it): the CBHG's recurrence is a bidirectional tf.contrib.rnn.LSTMCell (forget_bias 1.0, gates i | j | f | o).
    One decoder step at a small configuration against autograd on the float64 oracle with the same dropout masks and
    the device's relu / pool routing: losses 1e-5, every gradient element 1e-4 of its tensor's maximum -- including
    the LSTM cell kernels and biases of both directions and both stages --; then Adam steps reduce the loss and the
    checkpoint carries the cells under TF's names.  (TF's LSTMCell itself is recalled from its published source:
    parity unpinned, as for the inference path.)"""
    import tf_bundle
    from decoder import decoder_specs
    cfg = _cfg()
    cfg.update(use_lstm=True, model_path=str(tmp_path))
    dec = decoder_specs(cfg, None, None)
    rng = np.random.RandomState(8)
    for n, v in list(dec.store.vars.items()):            # (Glorot kernels from the constructor; everything else perturbed)
        if n.endswith('bias') or n.endswith('beta') or n.endswith('moving_mean'):
            dec.store.assign(n, rng.uniform(-0.2, 0.2, tuple(v.shape)).astype(np.float32))
        elif n.endswith('gamma') or n.endswith('moving_variance'):
            dec.store.assign(n, rng.uniform(0.5, 1.5, tuple(v.shape)).astype(np.float32))
    w = {k: v.cpu().numpy().copy() for k, v in dec.store.vars.items()}
    ppg = torch.softmax(torch.from_numpy(rng.standard_normal((4, 40, 61)) * 2), -1).float().numpy()
    t_mel = rng.uniform(0, 0.8, (4, 40, 80)).astype(np.float32)
    t_stft = rng.uniform(0, 0.8, (4, 40, 201)).astype(np.float32)
    cell = 'decoder/step2/CBHG/lstm/bidirectional_rnn/bw/lstm_cell'
    assert cell + '/kernel' in dec.store.vars and not any('/gru/' in n for n in dec.store.vars)
    H2 = cfg['steps_v'][1]['embed_size'] // 2
    assert tuple(dec.store.vars[cell + '/kernel'].shape) == (2 * H2, 4 * H2)
    tr = dec._get_trainer()
    tr.export_routing = True
    losses = tr.forward_backward(*(torch.from_numpy(a).cuda() for a in (ppg, t_mel, t_stft))).cpu().numpy()
    g_dev = {n: tr.g(n).cpu().numpy().astype(np.float64) for n in tr.names}
    ml, sl, grads, stats, ym, ys = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed, routing=_device_routing(tr))
    assert abs(losses[0] - ml) < 1e-5 * max(1, ml) and abs(losses[1] - sl) < 1e-5 * max(1, sl), (losses, ml, sl)
    assert np.abs(tr.y_stft.cpu().numpy().reshape(ys.shape) - ys).max() < 1e-4
    assert np.abs(grads[cell + '/kernel']).max() > 0 and np.abs(grads[cell + '/bias']).max() > 0
    _compare_gradients(tr, g_dev, grads)
    r1 = dec.exec_train_step(ppg, t_mel, t_stft)
    for _ in range(10):
        r = dec.exec_train_step(ppg, t_mel, t_stft)
    assert np.isfinite(r[2]) and r[2] < r1[2]
    dec.save(verbose=False)
    ck = tf_bundle.read_bundle(tf_bundle.latest_checkpoint(str(tmp_path)))
    assert ck[cell + '/kernel'].shape == (2 * H2, 4 * H2) and 'dec_opt/' + cell + '/bias/Adam_1' in ck


def test_adam_update_and_second_step():
    cfg = _cfg()
    dec, w, ppg, t_mel, t_stft = _setup(cfg)
    tr = dec._get_trainer()
    r1 = dec.exec_train_step(ppg, t_mel, t_stft)
    assert r1[3] == 1 and r1[4] is None and abs(r1[2] - (r1[0] + r1[1])) < 1e-5
    # oracle: same gradients -> tf.train.AdamOptimizer update (eps outside the bias correction)
    ml, sl, grads, stats, _, _ = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed)
    assert abs(r1[0] - ml) < 1e-4 * max(1, ml)
    for n in ('decoder/step2/y_logits/kernel', 'decoder/step1/CBHG/conv1d_banks/num_3/conv1d/conv1d/kernel',
              'decoder/step1/CBHG/gru/bidirectional_rnn/bw/gru_cell/candidate/kernel', 'decoder/step2/prenet/dense1/bias'):
        p, m, v = mo.adam_step(torch.from_numpy(w[n]).double(), torch.from_numpy(grads[n]), 0.0, 0.0, 1, 1e-3)
        got = dec.store.vars[n].cpu().numpy()
        assert np.abs(got - p.numpy()).max() < 5e-6, n       # |update| ~ lr = 1e-3
    r2 = dec.exec_train_step(ppg, t_mel, t_stft)
    assert r2[3] == 2 and np.isfinite(r2[2])
    # ten more steps on the same batch must reduce the loss (sanity of the whole loop)
    for _ in range(10):
        r = dec.exec_train_step(ppg, t_mel, t_stft)
    assert r[2] < r1[2]


def test_train_checkpoint_has_adam_slots(tmp_path):
    import tf_bundle
    cfg = _cfg()
    cfg['model_path'] = str(tmp_path)
    dec, w, ppg, t_mel, t_stft = _setup(cfg)
    dec.exec_train_step(ppg, t_mel, t_stft)
    dec.save(verbose=False)
    ck = tf_bundle.read_bundle(tf_bundle.latest_checkpoint(str(tmp_path)))
    assert int(ck['dec_opt/global_step']) == 1
    k = 'decoder/step1/prenet/dense1/kernel'
    assert ck['dec_opt/' + k + '/Adam'].shape == ck[k].shape and np.abs(ck['dec_opt/' + k + '/Adam_1']).max() > 0


def test_restore_resumes_adam_state_and_step(tmp_path, capsys):
    """save -> restore -> one step equals the uninterrupted run: tf.train.Saver brings back the Adam slots
    (dec_opt/<var>/Adam, Adam_1) and global_step with the weights (decoder.py:309-324).  Without them the first
    update after a resume is ~3x lr (m = v = 0 at a bias correction of ~1) and differs at the 1e-3 level."""
    cfg = _cfg()
    cfg['model_path'] = str(tmp_path)
    dec, w, ppg, t_mel, t_stft = _setup(cfg)
    for _ in range(2):
        dec.exec_train_step(ppg, t_mel, t_stft)
    dec.save(verbose=False)
    r3 = dec.exec_train_step(ppg, t_mel, t_stft)
    want = {n: v.clone() for n, v in dec.store.vars.items()}
    want_m = dec._trainer.m.clone()

    def check(d, what):
        worst = max(float((d.store.vars[n] - want[n]).abs().max()) for n in want)
        assert worst < 2e-6, '%s: parameters differ from the uninterrupted run by %.3e' % (what, worst)
        assert float((d._trainer.m - want_m).abs().max()) < 1e-6 * max(1.0, float(want_m.abs().max()))

    # (a) restore into a fresh model: the trainer does not exist yet and picks the slots up when it is created
    cfg2 = _cfg()
    cfg2['model_path'] = str(tmp_path)
    dec2, _, _, _, _ = _setup(cfg2, seed=11)
    dec2.restore()
    assert dec2.i_global_step == 2 and int(dec2.opt_state['dec_opt/global_step']) == 2
    q3 = dec2.exec_train_step(ppg, t_mel, t_stft)
    assert q3[3] == 3 and abs(q3[2] - r3[2]) < 1e-4 * max(1.0, abs(r3[2]))
    check(dec2, 'fresh model')
    # (b) restore into a model whose trainer already exists (its step count and slots were stale)
    dec2.restore()
    assert dec2._trainer.step_count == 2
    q3 = dec2.exec_train_step(ppg, t_mel, t_stft)
    assert q3[3] == 3
    check(dec2, 'existing trainer')


class _FakeDS:
    """The two methods decoder.train() calls on its dataset (decoder.py:381-398), over fixed random batches."""

    def __init__(self, n_windows, T):
        self.n, self.T = n_windows, T

    def get_n_windows(self, prop_val, **kw):
        return self.n, 2

    def spec_window_sampler(self, batch_size, n_epochs, randomize_samples, sample_trn, prop_val, **kw):
        rng = np.random.RandomState(1 if sample_trn else 2)
        while True:
            yield (torch.softmax(torch.from_numpy(rng.standard_normal((batch_size, self.T, 61)) * 2), -1).float().numpy(),
                   rng.uniform(0, 0.8, (batch_size, self.T, 80)).astype(np.float32),
                   rng.uniform(0, 0.8, (batch_size, self.T, 201)).astype(np.float32))


def test_train_loop_runs_through_a_save_epoch(tmp_path, monkeypatch, capsys):
    """decoder.train() (decoder.py:379-444) on a tiny dataset: two steps per epoch, a checkpoint and a validation
    batch every epoch -- the validation batch is evaluated on the TRAINING graph (decoder.py:349-353, 425-428), i.e.
    through the trainer's forward without a backward pass -- two epochs, then 'End of Training'."""
    import tf_bundle
    from decoder import decoder_specs
    cfg = _cfg()
    cfg.update(model_path=str(tmp_path), batch_size=2, n_epochs=2, save_each_n_epochs=1, ds_prop_val=0.3,
               randomize_samples=True)
    dec = decoder_specs(cfg, _FakeDS(4, cfg['input_shape'][0]), None)
    dec.store.load_dict(mo.init_weights(cfg, 'decoder', seed=5, perturb_bn=True))
    monkeypatch.setattr('builtins.input', lambda *a: '')
    dec.train()
    out = capsys.readouterr().out
    assert out.count('mel_loss_val=') == 2 and out.count('mel_loss_trn=') == 4 and 'End of Training !!!' in out
    assert dec.i_epoch == 2 and int(dec.opt_state['dec_opt/global_step']) == 4
    ck = tf_bundle.read_bundle(tf_bundle.latest_checkpoint(str(tmp_path)))
    assert int(ck['dec_opt/global_step']) == 4
    # metrics on a training model: no gradient is written, no step is taken, the moving averages move
    tr = dec._trainer
    tr.grad.fill_(7.0)
    mm = 'decoder/step1/CBHG/conv1d_1/moving_mean'
    before = dec.store.vars[mm].clone()
    rng = np.random.RandomState(5)
    b = next(dec.ds.spec_window_sampler(2, 1, True, False, 0.3))
    ml, sl, l = dec.exec_calc_metrics(*b)
    assert np.isfinite(l) and abs(l - (ml + sl)) < 1e-5 * max(1.0, l)
    assert float(tr.grad.min()) == 7.0 and tr.step_count == 4
    assert not torch.equal(dec.store.vars[mm], before)
    # and it is the train-mode forward: equal to forward_backward's losses on the same batch and dropout seed
    ref = tr.forward_backward(*(torch.from_numpy(a).cuda() for a in b)).cpu().numpy()
    assert abs(ref[0] - ml) < 1e-6 * max(1.0, ml)       # (moving averages do not enter the train-mode forward)


def _hp_cfg(seed=77):
    import os
    from conftest import ROOT
    cfg = json.load(open(os.path.join(ROOT, 'speech-cloner_amd', 'hp', 'decoder_cfg_d.json')))
    cfg.update(is_training=True, dropout_seed=seed)
    return cfg


def _compare_gradients(tr, g_dev, grads, tol_max=1e-4, tol_l2=1e-4):
    """Every tensor, every element: |dev - ref| <= tol_max x the tensor's max |ref|, and tol_l2 in relative L2."""
    assert set(grads) == set(tr.names)
    worst, worst_l2 = ('', 0.0), ('', 0.0)
    for n in tr.names:
        ref = grads[n]
        assert g_dev[n].shape == ref.shape, n
        err = float(np.abs(g_dev[n] - ref).max() / max(np.abs(ref).max(), 1e-6))
        l2 = float(np.linalg.norm(g_dev[n] - ref) / max(np.linalg.norm(ref), 1e-12))
        if err > worst[1]:
            worst = (n, err)
        if l2 > worst_l2[1]:
            worst_l2 = (n, l2)
    print('worst gradient mismatch %s %.3e; worst relative L2 %s %.3e' % (worst + worst_l2))
    assert worst[1] < tol_max, 'worst gradient mismatch %s: %.3e' % worst
    assert worst_l2[1] < tol_l2, 'worst relative L2 gradient error %s: %.3e' % worst_l2


@pytest.mark.parametrize('f16x3', [True, False])
def test_hp_size_train_step_matches_autograd(f16x3):
    """SURVEY section 8 row a23 at the SHIPPED sizes (hp/decoder_cfg_d.json: E = 256 / 512, K = 32 banks, 4 / 6
    highway layers, T = 400; /root/reference/decoder.py:185-263, 327-345): one decoder step on 2 windows -- both
    losses, every gradient (grouped K = 32 weight-gradient launches, H = 128 / 256 recurrences through time), the
    moving statistics and one Adam update -- against autograd on the float64 oracle with the same dropout masks.
    Tolerances: losses 1e-5 relative, outputs 1e-4, Adam 5e-6, and EVERY element of EVERY gradient tensor within 1e-4 of
    the tensor's max |gradient| (and the tensor 1e-4 in relative L2 norm) -- no exceptions, and 20x tighter than the
    2e-3 this test used to state (measured on MI355X: worst 8.8e-6 / 7.4e-6).

    What makes that possible: a relu sees millions of pre-activations per layer, and a handful lie within float32
    rounding of the kink (likewise two pooled neighbours within rounding of each other), where a float32 forward and a
    float64 one legitimately route the upstream gradient differently; one such element moves its unit's weight
    gradients by ~1 / sqrt(frames) of their size (round 2 measured 4-8 bank channels per stage 0.5-1.5 % off at 800
    frames and excused them; at 12,800 frames the first projection's and the prenet's relus showed 3e-3 / 1e-3 the
    same way).  Now the trainer exports the decisions its backward pass takes -- the filter bank's relu + max-pool and
    the first projection's relu (vc_bn_post_routing: the device function the backward kernels call), the prenet's relus
    (stored output > 0, as vc_relu_dropout_backward reads it), every highway block's relu (re-computed pre-activation
    > 0, as vc_highway_backward reads it) -- and the oracle takes them as GIVEN routing (model_oracle.dense /
    conv1d_banks / max_pool_2_same / cbhg): values move by at most the rounding that made the decision arbitrary, the
    gradients follow one route on both sides, and what is left is float32 summation error.

    f16x3: the filter bank and the first projection (forward, data gradients) as three float16 MFMA products of exactly
    split float32 operands (csrc/vc_gemm16.hip; the default) or, 'train_f16x3': False, on the f32-input MFMA kernels --
    the same bounds for both (measured: worst 4.5e-6 / 5.0e-6 on the split path, 8.0e-6 / 6.1e-6 on the f32-MFMA path)
    -- the filter gradients of this 800-frame batch stay on wgrad_kernel (frame count not a multiple of 64); the
    32-window test below runs them on the split path."""
    cfg = _hp_cfg()
    cfg['train_f16x3'] = f16x3
    assert cfg['steps_v'][0]['num_conv_banks'] == 32 and cfg['steps_v'][1]['embed_size'] == 512
    dec, w, ppg, t_mel, t_stft = _setup(cfg, N=2)
    tr = dec._get_trainer()
    tr.export_routing = True
    assert tr.f16x3 == f16x3
    assert tr.total == 33186713                                   # trainable parameters
    x = torch.from_numpy(ppg).cuda()
    losses = tr.forward_backward(x, torch.from_numpy(t_mel).cuda(), torch.from_numpy(t_stft).cuda())
    got = losses.cpu().numpy()
    g_dev = {n: tr.g(n).cpu().numpy().astype(np.float64) for n in tr.names}
    y_mel, y_stft = tr.y_mel.cpu().numpy(), tr.y_stft.cpu().numpy()
    moved = {n: dec.store.vars[n].cpu().numpy() for n in dec.store.vars if n in dec.store.non_trainable}
    p_before = {n: dec.store.vars[n].cpu().numpy().astype(np.float64) for n in
                ('decoder/step2/CBHG/conv1d_banks/num_32/conv1d/conv1d/kernel', 'decoder/step1/CBHG/conv1d_1/conv1d/kernel',
                 'decoder/step2/CBHG/gru/bidirectional_rnn/fw/gru_cell/gates/kernel', 'decoder/step1/y_logits/bias')}
    step = tr.apply_gradients(1)
    assert step == 1
    routing = _device_routing(tr)
    taps = {}
    ml, sl, grads, stats, ym, ys = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed, taps=taps, routing=routing)
    # the handed-in routing is the oracle's own wherever the decision is not a matter of rounding: it may differ from
    # max(pre, 0) / the true pool winner only where the float64 pre-activation is within 1e-4 of the kink or the tie
    for st_ in ('step1', 'step2'):
        pre = taps[st_]['banks_pre']
        on = routing[st_]['banks'][0].bool()
        flipped = on != (pre > 0)
        assert float(pre[flipped].abs().max()) < 1e-4 if flipped.any() else True
        assert flipped.float().mean() < 1e-4, float(flipped.float().mean())
    assert abs(got[0] - ml) < 1e-5 * max(1, ml) and abs(got[1] - sl) < 1e-5 * max(1, sl), (got, ml, sl)
    assert np.abs(y_mel.reshape(ym.shape) - ym).max() < 1e-4 * max(1.0, np.abs(ym).max())
    assert np.abs(y_stft.reshape(ys.shape) - ys).max() < 1e-4 * max(1.0, np.abs(ys).max())
    _compare_gradients(tr, g_dev, grads)
    for n, v in stats.items():
        assert np.abs(moved[n] - v.numpy()).max() < 1e-5 * max(1.0, float(v.abs().max())), n
    # Adam (tf.train.AdamOptimizer form) applied to the gradient the device computed: the first update is
    # lr * g / (|g| + ~3e-7), so for the few elements with |g| ~ 1e-7 it is the gradient's last bits, not the optimiser,
    # that a comparison through the ORACLE's gradient would test (the small configuration does that comparison)
    for n, p0 in p_before.items():
        p, m, v = mo.adam_step(torch.from_numpy(p0), torch.from_numpy(g_dev[n]), 0.0, 0.0, 1, 1e-3)
        assert np.abs(dec.store.vars[n].cpu().numpy() - p.numpy()).max() < 5e-6, n


def test_bench_shape_train_step_matches_autograd():
    """BASELINE configs[4]'s per-GPU shape -- 32 windows x 400 frames at the shipped sizes, the batch bench.py's train
    workload times (/root/reference/decoder.py:75-199, 327-345) -- against the float64 oracle's forward + autograd
    backward on the WHOLE batch (a minute of CPU on the GPU box): both losses 1e-5, outputs 1e-4, every element of every
    gradient tensor within 1e-4 of its tensor's max and 1e-4 in relative L2 (measured: 7.3e-6 / 6.0e-6), the moving
    statistics 1e-5.  This is the launch set the oracle had never seen:
    12,800-frame reductions in the weight-gradient kernels (frame-split, atomics), 3,200-block batch-norm statistics,
    32-window recurrences, the summed-groups data gradient of the banks, weight gradients on the side stream.  Relu /
    pool routing is the device's own (see test_hp_size_train_step_matches_autograd)."""
    cfg = _hp_cfg()
    dec, w, ppg, t_mel, t_stft = _setup(cfg, N=32)
    tr = dec._get_trainer()
    tr.export_routing = True
    args = [torch.from_numpy(a).cuda() for a in (ppg, t_mel, t_stft)]
    got = tr.forward_backward(*args).cpu().numpy()
    g_dev = {n: tr.g(n).cpu().numpy().astype(np.float64) for n in tr.names}
    y_mel, y_stft = tr.y_mel.cpu().numpy(), tr.y_stft.cpu().numpy()
    moved = {n: dec.store.vars[n].cpu().numpy() for n in dec.store.vars if n in dec.store.non_trainable}
    routing = _device_routing(tr)
    tr.routing = {}
    torch.cuda.empty_cache()
    ml, sl, grads, stats, ym, ys = _oracle_step(cfg, w, ppg, t_mel, t_stft, tr.seed, routing=routing)
    assert abs(got[0] - ml) < 1e-5 * max(1, ml) and abs(got[1] - sl) < 1e-5 * max(1, sl), (got, ml, sl)
    assert np.abs(y_mel.reshape(ym.shape) - ym).max() < 1e-4 * max(1.0, np.abs(ym).max())
    assert np.abs(y_stft.reshape(ys.shape) - ys).max() < 1e-4 * max(1.0, np.abs(ys).max())
    _compare_gradients(tr, g_dev, grads)
    for n, v in stats.items():
        assert np.abs(moved[n] - v.numpy()).max() < 1e-5 * max(1.0, float(v.abs().max())), n


def test_hp_size_split_weight_gradients_equal_unsplit_at_32_windows():
    """BASELINE configs[4]'s per-GPU shape (32 windows x 400 frames, shipped sizes): the weight-gradient launches split
    their frame reduction over workgroups and add partial sums with atomics (splits_allowed); that must equal the
    unsplit, fixed-order reduction within float32 summation noise (1e-4 of each tensor's max |gradient|; 12,800-frame
    sums), and the loss must not depend on it at all."""
    import training
    cfg = _hp_cfg()
    dec, w, ppg, t_mel, t_stft = _setup(cfg, N=32)
    tr = dec._get_trainer()
    args = [torch.from_numpy(a).cuda() for a in (ppg, t_mel, t_stft)]
    res = {}
    try:
        for splits in (1, 0):
            training._Ops.splits_allowed = splits
            l = tr.forward_backward(*args).cpu().numpy().copy()
            res[splits] = (l, tr.grad.clone())
    finally:
        training._Ops.splits_allowed = 1
    assert np.array_equal(res[0][0], res[1][0]) and np.isfinite(res[0][0]).all()
    worst = ('', 0.0)
    for n in tr.names:
        off, k, _ = tr.offsets[n]
        a, b = res[1][1][off:off + k], res[0][1][off:off + k]
        err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))
        if err > worst[1]:
            worst = (n, err)
    print('split vs unsplit weight gradients: worst %s %.3e' % worst)
    assert worst[1] < 1e-4, worst
    # moving statistics moved twice by the same batch: finite and changed (the step is usable at this shape)
    r = dec.exec_train_step(ppg, t_mel, t_stft)
    assert r[3] == 1 and np.isfinite(r[2])


_DP_WORKER = r'''
import os, sys, json
import numpy as np, torch
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'speech-cloner_amd')); sys.path.insert(0, os.path.join(root, 'tests'))
import dist_util
from test_training_gpu import _cfg, _setup
rank, world = dist_util.init('gloo')           # 2 ranks share the one GPU of the test box -> gloo moves the CUDA buffers
torch.cuda.set_device(0)
import training
training._Ops.splits_allowed = 0               # fixed summation order in every gradient kernel: this test is about the
                                               # exchange, and compares gradients computed twice to 1e-6
cfg = _cfg()
dec, w, _, _, _ = _setup(cfg)
rng = np.random.RandomState(100 + rank)
def batch(r):
    g = np.random.RandomState(100 + r)
    ppg = torch.softmax(torch.from_numpy(g.standard_normal((4, 40, 61)) * 2), -1).float().numpy()
    return ppg, g.uniform(0, 0.8, (4, 40, 80)).astype(np.float32), g.uniform(0, 0.8, (4, 40, 201)).astype(np.float32)
tr = dec._get_trainer()
mine = batch(rank)
tr.overlap_allreduce = False                    # this rank's own gradient, nothing on the wire yet
tr.forward_backward(*(torch.from_numpy(a).cuda() for a in mine))
g_local = tr.grad.clone()
p_before = tr.flat.clone()
tr.overlap_allreduce = True                     # the shipped form: stage 2's bucket travels under stage 1's backward
tr.forward_backward(*(torch.from_numpy(a).cuda() for a in mine))
assert len(tr._pending) == 2, tr._pending
tr.apply_gradients(world)                       # waits for the buckets; Adam with grad_scale 1/world
# reference on every rank: the other rank's gradient computed locally with identical weights/seeds
dec2, _, _, _, _ = _setup(_cfg())
tr2 = dec2._get_trainer()
tr2.overlap_allreduce = False
other = batch(1 - rank)
tr2.forward_backward(*(torch.from_numpy(a).cuda() for a in other))
total = g_local + tr2.grad
err = float((tr.grad - total).abs().max() / total.abs().max())
# Adam step from the averaged gradient
m = 0.1 * (total / world); v = 0.001 * (total / world) ** 2
lr_t = 1e-3 * (1 - 0.999) ** 0.5 / (1 - 0.9)
p_ref = p_before - lr_t * m / (v.sqrt() + 1e-8)
perr = float((tr.flat - p_ref).abs().max())
flat = dist_util.gather_concat(tr.flat[:1000].cpu().numpy().reshape(1, -1))
same = bool(np.array_equal(flat[0], flat[1]))   # replicas stay bit-identical after the update
if rank == 0:
    print('DP_RESULT', json.dumps({'grad_err': err, 'param_err': perr, 'replicas_equal': same}))
dist_util.finalize()
'''


def test_data_parallel_two_ranks(tmp_path):
    """BASELINE config 5 shape of the exchange: each rank trains on its own batch, gradients are
    summed over ranks (all-reduce of the flat arena) and scaled by 1/world inside Adam; batch-norm
    statistics stay per replica.  Two processes share this box's single GPU, so the process group
    uses gloo here (the multi-GPU bench uses nccl = RCCL)."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    script = tmp_path / 'dp.py'
    script.write_text(_DP_WORKER)
    port = 29600 + (os.getpid() % 300)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port), str(script), ROOT]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    line = [l for l in r.stdout.splitlines() if l.startswith('DP_RESULT')]
    assert r.returncode == 0 and line, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(line[0].split(' ', 1)[1])
    assert res['grad_err'] < 1e-6 and res['param_err'] < 1e-6 and res['replicas_equal'], res


@pytest.mark.parametrize('N,T,H', [(3, 9, 64), (131, 7, 64), (259, 5, 128), (130, 6, 256)])
def test_training_recurrence_window_groups_match_autograd(N, T, H):
    """vc_gru_train_forward / vc_gru_backward (/root/reference/modules.py:168-204 under tf.gradients) at batch sizes that
    select the kernels which advance 2 or 4 windows per workgroup (more than 128 / 256 windows per GPU, ragged last
    group included; 3 windows: the one-window kernels): hidden states, saved gates, r*h, and the gradient w.r.t. the
    gate pre-activations against float64 autograd of the recurrence restated in train_kernels_ref.gru_train from the oracle's cell
    (model_oracle.gru_direction: r, u = sigmoid([x, h] Wg + bg); c = tanh([x, r*h] Wc + bc); h' = u h + (1 - u) c), with
    the input projections given.  Tolerance 2e-5 forward, 1e-4 of the gradient's max backward (float32 sums over H
    products per step, chained over T steps)."""
    import ctypes as C
    import _vc
    import train_kernels_ref
    rng = np.random.RandomState(N + H)
    M = N * T
    xp = torch.from_numpy(rng.standard_normal((M, 6 * H)) * 0.5)
    wh = [torch.from_numpy(rng.standard_normal((H, 3 * H)) * (1.0 / np.sqrt(H))) for _ in range(2)]
    dG = torch.from_numpy(rng.standard_normal((M, 2 * H)))
    # float64 reference with autograd
    xr = xp.clone().requires_grad_(True)
    G_ref, _, _ = train_kernels_ref.gru_train(xr, wh, N, T, H)
    (G_ref * dG).sum().backward()
    # device
    f = lambda t: t.float().cuda().contiguous()
    xd, w0, w1, dGd = f(xp), f(wh[0]), f(wh[1]), f(dG)
    G = torch.empty((M, 2 * H), device='cuda')
    gates = torch.empty((2, M, 3 * H), device='cuda')
    rh = torch.empty((2, M, H), device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _vc.check(_vc.lib().vc_gru_train_forward(p(xd), p(w0), p(w1), N, T, H, p(G), p(gates), p(rh), _vc.current_stream()))
    dpre = torch.empty((M, 6 * H), device='cuda')
    w0t, w1t = w0.t().contiguous(), w1.t().contiguous()
    _vc.check(_vc.lib().vc_gru_backward(p(dGd), p(G), p(gates), p(w0), p(w1), p(w0t), p(w1t), N, T, H, p(dpre), _vc.current_stream()))
    torch.cuda.synchronize()
    assert float((G.cpu().double() - G_ref.detach()).abs().max()) < 2e-5
    gref = xr.grad
    err = float((dpre.cpu().double() - gref).abs().max() / gref.abs().max())
    assert err < 1e-4, err
    # saved gates (r | u | c) and r*h of the forward direction at the first step: h = 0 there
    x0 = xp.view(N, T, 6 * H)[:, 0, :3 * H]
    g0 = gates[0].view(N, T, 3 * H)[:, 0].cpu().double()
    assert float((g0[:, :2 * H] - torch.sigmoid(x0[:, :2 * H])).abs().max()) < 2e-6
    assert float((g0[:, 2 * H:] - torch.tanh(x0[:, 2 * H:])).abs().max()) < 2e-6
    assert float(rh[0].view(N, T, H)[:, 0].abs().max()) == 0.0


def test_encoder_train_step_matches_autograd(golden_dir):
    """Encoder training (encoder.py:134-194, 256-297) at the shipped
    hyper-parameters (E = 80, K = 6, 61 classes, 400 frames) starting from the reference's real
    enc_14 weights: loss / accuracy / mse, every gradient, and the Adam resume from the
    checkpoint's own slots.  Relu / max-pool routing is the device's own (see
    test_hp_size_train_step_matches_autograd): every element of every gradient within 1e-4 of its tensor's maximum
    (it was 3e-3 with the oracle routing by itself) -- at 2 windows and at the training batch of the shipped
    configuration, 32 windows.  The windows are the golden ones at their natural amplitude, shifted in time: with the
    same windows scaled to 0.5-1.0 the TRAINED recurrence has, in one window of 32, a stretch where it amplifies
    differences (float32 against float64: 7e-7 in the state at step 0, x10 every ~35 steps from step 100 on, 4e-4 at
    step 399 -- smooth exponential growth from rounding level, measured on the saved gates), and a comparison of a
    float32 trajectory with a float64 one then measures the number format, not the kernels."""
    import os
    from conftest import ROOT
    from encoder import encoder_spec_phn
    import tf_bundle
    cfg = json.load(open(os.path.join(ROOT, 'speech-cloner_amd', 'hp', 'encoder_cfg_d.json')))
    cfg.update(is_training=True, model_path=os.path.join(golden_dir, 'enc_14_ckpt'), dropout_seed=5)
    enc = encoder_spec_phn(cfg, None)
    enc.restore()
    g = np.load(os.path.join(golden_dir, 'encoder_fwd.npz'))
    w = tf_bundle.read_bundle(os.path.join(golden_dir, 'enc_14_ckpt', 'encoder-136512'))
    w = {k: v for k, v in w.items() if k.startswith('encoder/')}
    tr = enc._get_trainer()
    tr.export_routing = True
    keep = 1.0 - cfg['dropout_rate']
    for N in (2, cfg['batch_size']):
        rng = np.random.RandomState(4 + N)
        x = np.stack([np.roll(g['x'][i % 3], 16 * int(rng.randint(0, 25)), axis=0) for i in range(N)]).astype(np.float32)
        labels = rng.randint(0, 61, (N, 400))
        target = np.eye(61, dtype=np.float32)[labels]
        M = N * 400
        out3 = tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(target).cuda())
        rt = _device_routing(tr)['encoder']
        sb = tr.seed + 1000 * tr.step_count
        masks = (torch.from_numpy(_mask(M, 80, 80, sb + 1, keep)).view(N, 400, 80),
                 torch.from_numpy(_mask(M, 40, 40, sb + 2, keep)).view(N, 400, 40))
        wt = mo.to_torch(w, torch.float64, requires_grad=True)
        stats = {}
        lg, _, _, _ = mo.encoder_forward(torch.from_numpy(x).double(), wt, cfg, is_training=True, masks=masks, stats_out=stats,
                                         routing=rt)
        loss = mo.encoder_loss(lg, torch.from_numpy(target).double())
        acc, mse = mo.encoder_metrics(lg.detach(), torch.from_numpy(target).double())
        loss.backward()
        got = out3.cpu().numpy()
        assert abs(got[0] - float(loss.detach())) < 1e-5 * max(1.0, float(loss.detach())), (got, float(loss.detach()))
        assert abs(got[1] - float(acc)) < 1e-6 + 1.0 / M and abs(got[2] - float(mse)) < 1e-6
        worst = ('', 0.0)
        for n in tr.names:
            ref = wt[n].grad.numpy()
            err = np.abs(tr.g(n).cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-7)
            if err > worst[1]:
                worst = (n, err)
        print('encoder N=%d: worst gradient mismatch %s %.3e' % ((N,) + worst))
        assert worst[1] < 1e-4, 'N=%d: worst gradient mismatch %s: %.3e' % ((N,) + worst)
        # (the moving statistics this forward produced, against the oracle's from the same starting values)
        for n_, v_ in stats.items():
            assert np.abs(enc.store.vars[n_].cpu().numpy() - v_.numpy()).max() < 1e-5 * max(1.0, float(v_.abs().max())), n_
        w.update({n_: v_.numpy().astype(np.float32) for n_, v_ in stats.items()})       # the device moved them in place
    # a full step resumes Adam from the reference's own slots (beta powers are 0 after 136k steps)
    r = enc.exec_train_step(x[:2], target[:2])
    assert r[3] == 136513 and r[4] is None and np.isfinite(r[0])
    a_, m_, l_ = enc.exec_calc_metrics(x[:2], target[:2])
    assert 0.0 <= a_ <= 1.0 and np.isfinite(l_)


def test_weight_layouts_in_one_launch():
    """vc_weight_layouts: the forward ([cout, k*cin]) and data-gradient ([cin, k*cout], taps reversed) copies of many
    convolution kernels in one launch are exactly the torch transposes / flips the trainer used to launch one by one
    (ragged sizes, k = 1 .. 32), and a trainer's second step -- the first that runs on the refreshed copies -- gives the
    same losses as a trainer that rebuilds every copy with torch."""
    import ctypes as C
    import _vc
    rng = np.random.RandomState(3)
    shapes = [(1, 61, 256), (3, 4096, 128), (32, 256, 128), (7, 40, 40), (2, 33, 65), (5, 128, 256)]
    items, checks = [], []
    for k, cin, cout in shapes:
        W = torch.from_numpy(rng.standard_normal((k, cin, cout)).astype(np.float32)).cuda()
        fwd = torch.full((cout, k * cin), float('nan'), device='cuda')
        dg = torch.full((cin, k * cout), float('nan'), device='cuda')
        items += [_vc.LayoutItem(W.data_ptr(), fwd.data_ptr(), k, cin, cout, 0), _vc.LayoutItem(W.data_ptr(), dg.data_ptr(), k, cin, cout, 1)]
        checks.append((W, fwd, dg))
    arr = (_vc.LayoutItem * len(items))(*items)
    tab = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
    _vc.check(_vc.lib().vc_weight_layouts(C.c_void_p(tab.data_ptr()), len(items), _vc.current_stream()))
    torch.cuda.synchronize()
    for W, fwd, dg in checks:
        k, cin, cout = W.shape
        assert torch.equal(fwd, W.reshape(k * cin, cout).t().contiguous())
        assert torch.equal(dg, W.flip(0).permute(1, 0, 2).reshape(cin, k * cout).contiguous())
    # two steps with and without the in-place refresh
    import training
    cfg = _cfg()
    rng = np.random.RandomState(9)
    ppg = torch.softmax(torch.from_numpy(rng.standard_normal((4, 40, 61)) * 2), -1).float().cuda()
    mel = torch.from_numpy(rng.uniform(0, 0.8, (4, 40, 80)).astype(np.float32)).cuda()
    stft = torch.from_numpy(rng.uniform(0, 0.8, (4, 40, 201)).astype(np.float32)).cuda()
    out = []
    training._Ops.splits_allowed = 0            # fixed summation order in the gradient kernels: the two runs must agree exactly
    try:
        for refresh in (True, False):
            dec, _, _, _, _ = _setup(_cfg())
            tr = dec._get_trainer()
            if not refresh:
                tr._refresh_conv_layouts = lambda: None
            losses = []
            for _ in range(3):
                l = tr.forward_backward(ppg, mel, stft).clone()
                tr.apply_gradients(1)
                losses.append(l.cpu().numpy())
            out.append(np.stack(losses))
    finally:
        training._Ops.splits_allowed = 1
    assert np.array_equal(out[0], out[1]), (out[0], out[1])
