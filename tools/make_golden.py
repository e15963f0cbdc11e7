#!/usr/bin/env python
"""Regenerates the committed fixtures under tests/golden/ (run in the build container, where
/root/reference exists; the GPU box only ever sees the committed outputs).

  tests/golden/enc_14_ckpt/          trimmed copy of the reference's trained encoder checkpoint:
                                     the 38 model tensors + 5 optimiser scalars of
                                     /root/reference/enc_14_ckpt/encoder-136512 re-written as a
                                     TF bundle by speech-cloner_amd/tf_bundle.py (Adam slots
                                     dropped: 2.9 MB -> 1 MB).  Data only; every tensor's CRC32C
                                     is verified against the reference's index while reading.
  tests/golden/frontend_*.npz        seeded synthetic audio + the CPU oracle's features
                                     (oracle/frontend_oracle.py; "parity unpinned", see its header)
  tests/golden/encoder_fwd.npz       seeded features + oracle encoder outputs with enc_14 weights
                                     (CBHG_out in encoder_fwd_cbhg.npz)
  tests/golden/decoder_fwd_small.npz small-config decoder: seeded weights/inputs + oracle outputs
                                     (stage 2's weights in decoder_fwd_small_step2.npz)
  tests/golden/reference_hp/,        verbatim copies for the reference-facing CPU tests,
  tests/golden/reference_ckpt/       see make_reference_copies()
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'speech-cloner_amd'))

import tf_bundle                                   # noqa: E402
from oracle import frontend_oracle as fo           # noqa: E402
from oracle import model_oracle as mo              # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference'

FE_KW = dict(sr=16000, pre_emphasis=0.97, hop_length=80, win_length=400, n_mels=80, n_mfcc=40,
             n_fft=None, window='hann', mfcc_normaleze_first_mfcc=True, mfcc_norm_factor=0.01,
             calc_mfcc_derivate=True, M_dB_norm_factor=0.01, P_dB_norm_factor=0.01,
             mean_abs_amp_norm=0.003, clip_output=True)


def make_enc14():
    src = os.path.join(REF, 'enc_14_ckpt', 'encoder-136512')
    w = tf_bundle.read_bundle(src, verify_crc=True)
    keep = {k: v for k, v in w.items() if 'Adam' not in k and not k.startswith('opt/beta')}
    dst_dir = os.path.join(GOLD, 'enc_14_ckpt')
    os.makedirs(dst_dir, exist_ok=True)
    tf_bundle.write_bundle(os.path.join(dst_dir, 'encoder-136512'), keep)
    with open(os.path.join(dst_dir, 'checkpoint'), 'w') as f:
        f.write('model_checkpoint_path: "encoder-136512"\nall_model_checkpoint_paths: "encoder-136512"\n')
    # known-answer CRCs straight from the reference's own index
    ents = tf_bundle.list_bundle(src)
    kat = {k: int(ents[k].crc32c) for k in ('encoder/y_logits/bias', 'encoder/CBHG/conv1d_1/beta')}
    json.dump(kat, open(os.path.join(dst_dir, 'crc_kat.json'), 'w'))
    print('enc_14: kept %d tensors, %d floats' % (len(keep), sum(v.size for v in keep.values())))
    return keep


def make_frontend():
    # (a) shipped configuration, two ragged utterances
    wav = fo.synth_speech(2, 12000, seed=7)
    lens = np.array([12000, 9111], dtype=np.int32)
    outs = fo.calc_MFCC_input_batch(wav, lens, **FE_KW)
    np.savez_compressed(os.path.join(GOLD, 'frontend_default.npz'), wav=wav, lens=lens,
                        mfcc0=outs[0][0], mel0=outs[1][0], pdb0=outs[2][0],
                        mfcc1=outs[0][1], mel1=outs[1][1], pdb1=outs[2][1])
    # (b) non-default path (generic DFT kernel): n_fft 512 > win 400, hamming, no derivative,
    #     unit factors / no clip exercise the "== 1.0 skips" branches (audio_lib.py:125,223-235)
    kw = dict(FE_KW)
    kw.update(hop_length=40, win_length=400, n_fft=512, n_mels=64, n_mfcc=20, window='hamming',
              calc_mfcc_derivate=False, mfcc_norm_factor=1.0, M_dB_norm_factor=1.0,
              P_dB_norm_factor=1.0, clip_output=False, mfcc_normaleze_first_mfcc=False,
              pre_emphasis=0.0, mean_abs_amp_norm=1.0)
    rng = np.random.RandomState(11)
    wav2 = (0.1 * rng.standard_normal((1, 4000))).astype(np.float32)
    o2 = fo.calc_MFCC_input(wav2[0], **kw)
    np.savez_compressed(os.path.join(GOLD, 'frontend_generic.npz'), wav=wav2,
                        mfcc=o2[0], mel=o2[1], pdb=o2[2])
    print('frontend: default F=%s, generic F=%d' % ([o.shape[0] for o in outs[0]], o2[0].shape[0]))


def make_encoder(enc_w):
    enc_cfg = json.load(open(os.path.join(REF, 'hp', 'encoder_cfg_d.json')))
    wav = fo.synth_speech(3, 32000, seed=21)
    x = np.stack([fo.calc_MFCC_input(wav[i], **FE_KW)[0][:400] for i in range(3)]).astype(np.float32)
    for dt, tag in ((torch.float64, 'f64'),):
        wt = mo.to_torch({k: v for k, v in enc_w.items() if k.startswith('encoder/')}, dt)
        taps = {}
        lg, pr, cl, out = mo.encoder_forward(torch.from_numpy(x).to(dt), wt, enc_cfg, taps=taps)
    # two files, each under the 1 MiB limit of a committed file: CBHG_out lives on its own
    np.savez_compressed(os.path.join(GOLD, 'encoder_fwd.npz'), x=x,
                        y_logits=lg.numpy().astype(np.float32), y_pred=pr.numpy().astype(np.float32),
                        y_pred_class=cl.numpy(),
                        prenet=taps['prenet'].numpy().astype(np.float32),
                        highway=taps['highway'].numpy().astype(np.float32))
    np.savez_compressed(os.path.join(GOLD, 'encoder_fwd_cbhg.npz'), CBHG_out=out.numpy().astype(np.float32))
    print('encoder: logits', lg.shape, 'classes', np.unique(cl.numpy()).size)


def small_decoder_cfg():
    return {'model_name': 'decoder', 'input_shape': [40, 61], 'dropout_rate': 0.1, 'is_training': False,
            'use_Cudnn': False, 'use_lstm': False, 'use_target_mel_step2': False,
            'mel_loss_weight': 400, 'stft_loss_weight': 400, 'loss_type': 'sum',
            'steps_v': [{'embed_size': 64, 'num_conv_banks': 5, 'num_highwaynet_blocks': 2, 'n_output': 80},
                        {'embed_size': 96, 'num_conv_banks': 4, 'num_highwaynet_blocks': 1, 'n_output': 201}]}


def make_decoder_small():
    cfg = small_decoder_cfg()
    w = mo.init_weights(cfg, 'decoder', seed=5, perturb_bn=True)
    rng = np.random.RandomState(6)
    logits = rng.standard_normal((2, 40, 61)).astype(np.float32) * 2
    ppg = torch.softmax(torch.from_numpy(logits).double(), -1)
    ym, ys = mo.decoder_forward(ppg, mo.to_torch(w, torch.float64), cfg)
    # stage 2's weights in a second file (each file under the 1 MiB limit of a committed file)
    s2 = 'decoder/step2/'
    np.savez_compressed(os.path.join(GOLD, 'decoder_fwd_small.npz'), ppg=ppg.numpy().astype(np.float32),
                        y_mel=ym.numpy().astype(np.float32), y_stft=ys.numpy().astype(np.float32),
                        cfg=json.dumps(cfg), **{'w:' + k: v for k, v in w.items() if not k.startswith(s2)})
    np.savez_compressed(os.path.join(GOLD, 'decoder_fwd_small_step2.npz'),
                        **{'w:' + k: v for k, v in w.items() if k.startswith(s2)})
    print('decoder small:', ym.shape, ys.shape)


def make_reference_copies(enc_w):
    """What the reference-facing CPU tests read, so that they need nothing outside the repository:
      reference_hp/*.json            the reference's four hyper-parameter files, verbatim
      reference_ckpt/<ckpt>/         each checkpoint's TF-written .index (and `checkpoint` state file) verbatim, the
                                     tensors of its data blob as tensors_<i>.npz (< 1 MiB each; enc_14's 43 model
                                     tensors are those of golden enc_14_ckpt and are not repeated), and bundle.json
                                     with the blob's size and SHA-256, so that a test rebuilds the blob byte for byte
    """
    import hashlib
    import shutil
    hp_dir = os.path.join(GOLD, 'reference_hp')
    os.makedirs(hp_dir, exist_ok=True)
    for f in ('encoder_cfg_d.json', 'decoder_cfg_d.json', 'ds_enc_cfg_d.json', 'ds_dec_cfg_d.json'):
        shutil.copyfile(os.path.join(REF, 'hp', f), os.path.join(hp_dir, f))
    for ck, base, with_state in (('enc_14_ckpt', 'encoder-136512', True), ('enc_6_ckpt', 'encoder-184032', False),
                                 ('enc_2_ckpt', 'encoder-136152', False)):
        src = os.path.join(REF, ck, base)
        dst_dir = os.path.join(GOLD, 'reference_ckpt', ck)
        os.makedirs(dst_dir, exist_ok=True)
        shutil.copyfile(src + '.index', os.path.join(dst_dir, base + '.index'))
        if with_state:
            shutil.copyfile(os.path.join(REF, ck, 'checkpoint'), os.path.join(dst_dir, 'checkpoint'))
        blob = src + '.data-00000-of-00001'
        if not os.path.exists(blob):                   # enc_2_ckpt ships no data blob (.MISSING_LARGE_BLOBS)
            continue
        w = tf_bundle.read_bundle(src, verify_crc=True)
        shared = set(enc_w) if ck == 'enc_14_ckpt' else set()
        parts, cur, nbytes = [], {}, 0
        for k in tf_bundle.list_bundle(src):
            if k in shared:
                continue
            if cur and nbytes + w[k].nbytes > 900000:
                parts.append(cur)
                cur, nbytes = {}, 0
            cur[k] = w[k]
            nbytes += w[k].nbytes
        parts.append(cur)
        for i, p in enumerate(parts):
            np.savez_compressed(os.path.join(dst_dir, 'tensors_%d.npz' % i), **p)
        data = open(blob, 'rb').read()
        json.dump({'prefix': base, 'data_size': len(data), 'data_sha256': hashlib.sha256(data).hexdigest(),
                   'model_tensors_from': 'enc_14_ckpt' if shared else None},
                  open(os.path.join(dst_dir, 'bundle.json'), 'w'), indent=1)
        print('%s: %d tensors in %d file(s)' % (ck, sum(len(p) for p in parts), len(parts)))


if __name__ == '__main__':
    os.makedirs(GOLD, exist_ok=True)
    enc_w = make_enc14()
    make_frontend()
    make_encoder(enc_w)
    make_decoder_small()
    make_reference_copies(enc_w)
