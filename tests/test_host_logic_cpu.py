"""Host-side logic that needs no GPU: conversion framing (bit-exact vs the oracle), config
helpers, model-object construction / variable naming / checkpoint plumbing on a CPU
VariableStore, and the 2-process (gloo) sharding path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import conversion_oracle as co
from oracle import model_oracle as mo

HP = os.path.join(ROOT, 'speech-cloner_amd', 'hp')


def test_compound_bit_exact_and_covering():
    import conversion
    rng = np.random.RandomState(0)
    for N in range(2, 10):
        for T in (4, 8, 400, 402, 13):
            y0 = rng.standard_normal((N, T, 3))
            y1 = rng.standard_normal((N - 1, T, 3))
            a, b = conversion.compound(y0, y1), co.compound(y0, y1)
            assert a.shape == b.shape and np.array_equal(a, b), (N, T)
    # algebraic property: N*T frames, each from a window covering it
    N, T = 5, 400
    which, win, frame = conversion.compound_index(N, T)
    assert len(which) == N * T
    t_out = np.arange(N * T)
    start = np.where(which == 0, win * T, win * T + T // 2)
    assert np.array_equal(start + frame, t_out)


def test_window_plan_matches_reference_arithmetic():
    import conversion
    cfg = {'hop_length': 80, 'n_timesteps': 400, 'sample_rate': 16000}
    for n_frames in (641, 800, 801, 1200, 12001, 399):
        for t_s, t_e in ((0, 60), (5, 60), (0, 3), (2, 7)):
            total, n_s, n_e = co.window_plan(n_frames, 16000, 80, 400, t_s, t_e)
            if n_e <= n_s:
                with pytest.raises(Exception):
                    conversion.window_plan(n_frames, cfg, t_s, t_e)
                continue
            pad, s, e = conversion.window_plan(n_frames, cfg, t_s, t_e)
            assert (n_frames + pad, s, e) == (total, n_s, n_e)
            assert (e - s) % 400 == 0
    # config 1 of BASELINE.json: 3.2 s utterance -> 641 frames -> padded to 800 -> 2 windows
    pad, s, e = conversion.window_plan(641, cfg, 0, 60)
    assert (pad, s, e) == (159, 0, 800)


class _FakeDecoder:
    """decoder.predict stand-in: echoes a deterministic function of the input windows."""

    def predict(self, x, batch_size=32):
        from collections import namedtuple
        nt = namedtuple('predict', 'y_mel y_stft y_phn')
        return nt(x[..., :3] * 2.0, x[..., :5] + 1.0, x[..., :4] - 1.0)


def test_conversion2_stitching_end_to_end():
    import conversion
    cfg = {'hop_length': 80, 'n_timesteps': 400, 'sample_rate': 16000, 'win_length': 400, 'n_fft': None,
           'P_dB_norm_factor': 0.01, 'pre_emphasis': 0.97, 'mean_abs_amp_norm': 0.003}
    rng = np.random.RandomState(1)
    F = 1001
    mfcc, mel, stft = rng.standard_normal((F, 80)), rng.standard_normal((F, 80)), rng.standard_normal((F, 201))
    r = conversion.conversion2(_FakeDecoder(), mfcc, mel, stft, cfg, t_s=0, t_e=60, vocoder=None)
    assert r.mel_pred.shape == (1200, 3) and r.stft_pred.shape == (1200, 5) and r.phn_pred.shape == (1200, 4)
    assert r.y_wav_true is None and r.y_wav_pred is None
    # the echo decoder is pointwise, so stitching must reproduce the padded input exactly
    padded = np.concatenate([mfcc, np.zeros((199, 80))], 0)
    assert np.array_equal(r.mel_pred, padded[:, :3] * 2.0)
    assert np.array_equal(r.stft_true, np.concatenate([stft, np.zeros((199, 201))], 0))
    r1 = conversion.conversion(_FakeDecoder(), mfcc[:400], mel[:400], stft[:400], cfg, t_s=0, t_e=60, vocoder=None)
    assert r1.mel_pred.shape == (400, 3) and len(r1) == 6


def test_aux_func_config_roundtrip(tmp_path, capsys, monkeypatch):
    import aux_func
    p = str(tmp_path / 'a' / 'b' / 'cfg.json')
    d = {'x': 1, 'nested': {'k': [1, 2]}, 'name': 'enc'}
    aux_func.save_cfg_d(d, p)
    assert 'Salvando:' in capsys.readouterr().out
    assert aux_func.load_cfg_d(p) == d
    aux_func.save_cfg_d(d, p)                                   # unchanged -> no prompt, no rewrite
    d2 = dict(d, x=2)
    monkeypatch.setattr('builtins.input', lambda: 'n')
    aux_func.save_cfg_d(d2, p)
    assert aux_func.load_cfg_d(p)['x'] == 1
    monkeypatch.setattr('builtins.input', lambda: 'y')
    aux_func.save_cfg_d(d2, p)
    assert aux_func.load_cfg_d(p)['x'] == 2
    assert aux_func.show_diff({'a': 1, 'b': {'c': 1}}, {'a': 2, 'b': {'c': 2}, 'z': 0}) == 3


def test_hp_configs_keep_reference_key_sets(golden_dir):
    for f in ('encoder_cfg_d.json', 'decoder_cfg_d.json', 'ds_enc_cfg_d.json', 'ds_dec_cfg_d.json'):
        mine = json.load(open(os.path.join(HP, f)))
        ref = json.load(open(os.path.join(golden_dir, 'reference_hp', f)))      # the reference's hp/, verbatim
        assert mine == ref, f


def test_model_objects_on_cpu_store(golden_dir, capsys):
    """Construction creates exactly the reference's variables (names/shapes), restore() reads the
    TF bundle, the decoder constructor restores the encoder (decoder.py:57) -- no kernels run."""
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    ec = json.load(open(os.path.join(HP, 'encoder_cfg_d.json')))
    dc = json.load(open(os.path.join(HP, 'decoder_cfg_d.json')))
    ec.update(is_training=False, device='cpu', model_path=os.path.join(golden_dir, 'enc_14_ckpt'))
    dc.update(is_training=False)
    enc = encoder_spec_phn(ec, None)
    before = enc.store.vars['encoder/y_logits/bias'].clone()
    dec = decoder_specs(dc, None, enc)
    out = capsys.readouterr().out
    assert 'Restored:' in out and ' Encoder Restored !!!' in out
    assert not np.array_equal(before.numpy(), enc.store.vars['encoder/y_logits/bias'].numpy())
    exp = {n: tuple(s) for n, s, _ in mo.model_variable_shapes(ec, 'encoder') + mo.model_variable_shapes(dc, 'decoder')}
    got = {n: tuple(v.shape) for n, v in enc.store.vars.items()}
    assert got == exp
    n_dec = sum(v.numel() for n, v in enc.store.vars.items() if n.startswith('decoder/') and n not in enc.store.non_trainable)
    assert n_dec == 33186713
    assert dec.sess is enc.sess and dec.get_input_shape() == (400, 80)
    assert enc.get_outputs()._fields == ('y_pred', 'y_pred_class', 'y_logits', 'CBHG_out')
    # TF initialisers that matter (modules.py:317; GRUCell gate bias 1.0)
    assert float(enc.store.vars['decoder/step1/CBHG/highwaynet_0/dense2/bias'][0]) == -1.0
    assert float(enc.store.vars['decoder/step2/CBHG/gru/bidirectional_rnn/bw/gru_cell/gates/bias'][0]) == 1.0
    with pytest.raises(Exception, match='not in training'):
        dec.exec_train_step(None, None, None)                      # built with is_training = False


def test_use_cudnn_is_refused_not_ignored():
    """modules.py:188-197, 227-236: use_Cudnn builds CudnnGRU / CudnnLSTM (one opaque parameter blob); a checkpoint of
    such a model cannot be restored into the GRUCell / LSTMCell variables this package creates, so the constructors
    and the recurrence wrappers refuse the flag instead of building another model behind the caller's back."""
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    import modules
    ec = json.load(open(os.path.join(HP, 'encoder_cfg_d.json')))
    dc = json.load(open(os.path.join(HP, 'decoder_cfg_d.json')))
    ec.update(is_training=False, device='cpu', use_Cudnn=True)
    dc.update(is_training=False, device='cpu', use_Cudnn=True)
    with pytest.raises(NotImplementedError, match='use_Cudnn'):
        encoder_spec_phn(ec, None)
    with pytest.raises(NotImplementedError, match='use_Cudnn'):
        decoder_specs(dc, None, None)
    for fn in (modules.gru, modules.lstm):
        with pytest.raises(NotImplementedError, match='use_Cudnn'):
            fn(None, num_units=8, bidirection=True, use_Cudnn=True)
    with pytest.raises(NotImplementedError, match='use_Cudnn'):
        modules.CBHG(None, use_Cudnn=True, is_training=False)


def test_native_library_is_required():
    import _vc
    assert os.path.exists(_vc.LIB_PATH), 'libvc_hip.so must be built (no CPU fallback exists)'
    import audio_lib
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_vc.VCError):
            audio_lib.calc_MFCC_input(np.zeros(8000, dtype=np.float32))


def test_shard_range_partitions():
    import dist_util
    for n in (0, 1, 7, 32, 33, 64):
        for w in (1, 2, 3, 8):
            spans = [dist_util.shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, dist_util
rank, world = dist_util.init('gloo')
assert world == 2
lo, hi = dist_util.shard_range(5, rank, world)
x = np.arange(10, dtype=np.float32).reshape(5, 2)[lo:hi]
y = np.zeros((3, 2), np.float32); y[:hi - lo] = x * 2          # equal shapes for all_gather
dist_util.barrier()
m = dist_util.max_over_ranks(1.0 + rank)
g = dist_util.gather_concat(y)
if rank == 0:
    assert m == 2.0, m
    assert g.shape == (6, 2) and np.array_equal(g[:3], np.arange(6, dtype=np.float32).reshape(3, 2) * 2)
    assert np.array_equal(g[3:5], np.arange(6, 10, dtype=np.float32).reshape(2, 2) * 2)
    print('GLOO_OK')
dist_util.finalize()
'''


def test_two_process_gloo_sharding(tmp_path):
    script = tmp_path / 'w.py'
    script.write_text(_WORKER)
    port = 29500 + (os.getpid() % 500)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port), str(script),
           os.path.join(ROOT, 'speech-cloner_amd')]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and 'GLOO_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_dataset_filter_and_split_logic_match_oracle():
    """sound_ds.py:116-211 on the host (no GPU: the cache is not built)."""
    import sound_ds
    from oracle import dataset_oracle as do
    rng = np.random.RandomState(0)
    n = 57
    ds = {'wav': [np.zeros(int(L), np.float32) for L in rng.randint(1000, 90000, n)],
          'spk_id': np.array(['a', 'b', 'c', 'd'])[rng.randint(0, 4, n)],
          'ds_type': np.array(['TRAIN', 'TEST'])[rng.randint(0, 2, n)]}
    cfg = {'sample_rate': 16000, 'hop_length': 80, 'win_length': 400, 'n_mfcc': 40, 'n_timesteps': 400,
           'random_seed': 1, 'verbose': False, 'ds_norm': (0.0, 1.0)}
    d = sound_ds.Sound_DS(cfg, ds, build_cache=False)
    filters = [None, {}, {'spk_id': 'a'}, {'spk_id': ['a', 'c'], 'ds_type': 'TRAIN'}, {'spk_id': None, 'ds_type': 'TEST'}]
    for typ in ('trn', 'val', 'tst'):
        filters.append({'split_d': {'split_key': 'spk_id', 'split_type': typ, 'split_props_v': (0.6, 0.8)},
                        'spk_id': ['a', 'b', 'd']})
    for f in filters:
        assert np.array_equal(d.get_ds_filter(f), do.get_ds_filter(ds, f)), f
        if f is not None:
            assert d.get_n_windows(0.3, f) == do.get_n_windows(ds, cfg, 0.3, f)
    parts = [d.get_ds_filter({'split_d': {'split_key': 'spk_id', 'split_type': t, 'split_props_v': (0.6, 0.8)}})
             for t in ('trn', 'val', 'tst')]
    assert (parts[0].astype(int) + parts[1] + parts[2] == 1).all()           # a partition
    with pytest.raises(Exception, match='no encontrado'):
        d.get_ds_filter({'nope': 1})
    with pytest.raises(Exception, match='split no reconocido'):
        d.get_ds_filter({'split_d': {'split_key': 'spk_id', 'split_type': 'x', 'split_props_v': (0.1, 0.2)}})
    with pytest.raises(Exception, match='tupla de len 2'):
        d.get_ds_filter({'split_d': {'split_key': 'spk_id', 'split_type': 'trn', 'split_props_v': [0.1, 0.2]}})


def test_oracle_given_routing_reproduces_its_own_forward():
    """oracle/model_oracle.py: conv1d_banks(relu_on=...) / max_pool_2_same(winners=...) with the routing derived from
    the oracle's OWN pre-activations (the rule of vc_bn_post_routing, include/vc_hip.h: relu passes a > 0; a frame
    wins its own pool output when it is the last frame or >= its successor, the previous frame's when strictly greater
    than its predecessor) give exactly relu + max-pool, values and gradients."""
    import torch
    rng = np.random.RandomState(1)
    x = torch.from_numpy(rng.standard_normal((3, 17, 6))).requires_grad_(True)
    a = torch.relu(x)
    ref = mo.max_pool_2_same(a)
    g = torch.from_numpy(rng.standard_normal(ref.shape))
    (ref * g).sum().backward()
    gref = x.grad.clone()
    x.grad = None
    ad = a.detach()
    T = ad.shape[1]
    nxt = torch.cat([ad[:, 1:], ad[:, -1:]], 1)
    prv = torch.cat([ad[:, :1], ad[:, :-1]], 1)
    t = torch.arange(T)[None, :, None]
    on = ad > 0
    own = on & ((t == T - 1) | (ad >= nxt))
    prev = on & (t > 0) & (ad > prv)
    bits = on.to(torch.uint8) | (own.to(torch.uint8) << 1) | (prev.to(torch.uint8) << 2)
    r = mo.routing_from_bits(bits)
    y = mo.max_pool_2_same(x * r[0], r[1:])
    assert torch.equal(y.detach(), ref.detach())
    (y * g).sum().backward()
    assert torch.equal(x.grad, gref)


def test_gradient_buckets_cover_the_arena_exactly_once(monkeypatch):
    """Data-parallel exchange (training.py: _start_allreduce / _complete_exchange; decoder.py:236-246 analogue under
    DP): the two overlapped buckets of the decoder trainer (stage 2 first, then stage 1) plus whatever
    _complete_exchange sums itself must cover [0, total) of the flat gradient arena exactly once -- an element summed
    twice or never would train replicas apart silently.  Checked for both trainers at the shipped sizes with a
    recording stand-in for the process group (no GPU, no kernels: only the bookkeeping runs)."""
    import torch
    import training
    from encoder import encoder_spec_phn
    from decoder import decoder_specs
    ec = json.load(open(os.path.join(HP, 'encoder_cfg_d.json')))
    dc = json.load(open(os.path.join(HP, 'decoder_cfg_d.json')))
    ec.update(is_training=True, device='cpu')
    dc.update(is_training=True, device='cpu')
    calls = []

    class Work:
        waited = 0

        def wait(self):
            Work.waited += 1

    def fake_all_reduce(t, op=None, async_op=False):
        calls.append((t.data_ptr(), t.numel(), async_op))
        return Work() if async_op else None

    # host-only bookkeeping on CPU-device models, also on a machine with a GPU (which would otherwise hand the
    # trainers a device stream for a CPU device)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a: 2)
    monkeypatch.setattr(torch.distributed, 'all_reduce', fake_all_reduce)

    def covered(tr):
        base = tr.grad.data_ptr()
        spans = sorted(((p - base) // 4, (p - base) // 4 + n) for p, n, _ in calls)
        assert spans[0][0] == 0 and spans[-1][1] == tr.total, spans
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 == b0, 'gap or overlap between %s and %s' % ((a0, a1), (b0, b1))
        return spans

    # decoder: the two buckets forward_backward starts, in its order, then the completion
    dec = decoder_specs(dc, None, None)
    tr = training.DecoderTrainer(dec)
    assert tr.total == 33186713
    tr._start_allreduce(*tr._slice_of('decoder/step2/'))
    tr._start_allreduce(*tr._slice_of('decoder/step1/'))
    assert len(tr._pending) == 2 and all(c[2] for c in calls)
    tr._complete_exchange()
    spans = covered(tr)
    assert len(spans) == 2 and Work.waited == 2 and tr._pending == []         # nothing left for the gap filler
    assert spans[1][1] - spans[1][0] > spans[0][1] - spans[0][0]            # stage 2 (created last) is the larger bucket
    # only ONE bucket went out (e.g. an exception between the stages): the completion sums the rest itself
    calls.clear()
    tr._start_allreduce(*tr._slice_of('decoder/step2/'))
    tr._complete_exchange()
    assert len(covered(tr)) == 2 and [c[2] for c in calls] == [True, False]
    # overlap switched off: one blocking all-reduce of everything
    calls.clear()
    tr.overlap_allreduce = False
    tr._start_allreduce(*tr._slice_of('decoder/step2/'))
    tr._complete_exchange()
    assert covered(tr) == [(0, tr.total)]
    # a forward_backward that finds buckets nobody consumed waits for them before touching the arena
    tr.overlap_allreduce = True
    calls.clear()
    Work.waited = 0
    tr._start_allreduce(*tr._slice_of('decoder/step2/'))
    tr._drain_pending()
    assert Work.waited == 1 and tr._pending == []
    # encoder: starts no bucket -> the completion is one all-reduce of the whole arena
    calls.clear()
    enc = encoder_spec_phn(ec, None)
    te = training.EncoderTrainer(enc)
    te._complete_exchange()
    assert covered(te) == [(0, te.total)]


def test_scope_selective_invalidation_keeps_a_frozen_models_layout_copies():
    """A decoder trains on top of a frozen encoder in ONE VariableStore: after Adam only the decoder's kernel-layout
    copies are stale.  invalidate(prefix) drops exactly the cache entries whose scope lies under the prefix (and still
    bumps the version every outside cache checks); invalidate() drops everything."""
    import types
    import modules
    st = modules.VariableStore.__new__(modules.VariableStore)
    st._cache = {('conv', 'encoder/CBHG/conv1d_1'): 1, ('bn', 'encoder/prenet'): 2, ('dense', 'decoder/step1/prenet/dense1'): 3,
                 ('g16conv', 'decoder/step2/CBHG/conv1d_1', 'conv1d_1'): 4, ('eye', 80): 5, ('gru', 'decoder2/x'): 6,
                 ('lstm', 'decoder', True): 7}
    st.version = 3
    st.invalidate('decoder')
    assert set(st._cache) == {('conv', 'encoder/CBHG/conv1d_1'), ('bn', 'encoder/prenet'), ('eye', 80), ('gru', 'decoder2/x')}
    assert st.version == 4
    st.invalidate()
    assert st._cache == {} and st.version == 5
