"""TF-bundle checkpoint reader/writer (speech-cloner_amd/tf_bundle.py) -- CPU tests.

Known-answer pins come from the reference's own checkpoint index: the masked CRC32C values of
two tensors recorded in SURVEY.md section 8c, and the training-state scalars of section 5."""
import json
import os

import numpy as np
import pytest

import tf_bundle


def test_crc32c_known_answers():
    # RFC 3720 test vectors for CRC-32C
    assert tf_bundle.crc32c(b'123456789') == 0xE3069283
    assert tf_bundle.crc32c(bytes(32)) == 0x8A9136AA
    assert tf_bundle.crc32c(bytes([0xFF] * 32)) == 0x62A8AB43
    m = tf_bundle.mask_crc(0xE3069283)
    assert tf_bundle.unmask_crc(m) == 0xE3069283


def test_golden_enc14_bundle(golden_dir):
    d = os.path.join(golden_dir, 'enc_14_ckpt')
    prefix = tf_bundle.latest_checkpoint(d)
    assert prefix is not None and prefix.endswith('encoder-136512')
    ents = tf_bundle.list_bundle(prefix)
    kat = json.load(open(os.path.join(d, 'crc_kat.json')))
    # masked CRC32C known answers from the reference's own index
    assert kat == {'encoder/y_logits/bias': 2862092325, 'encoder/CBHG/conv1d_1/beta': 4159623088}
    for k, v in kat.items():
        assert ents[k].crc32c == v
    w = tf_bundle.read_bundle(prefix, verify_crc=True)
    model = {k: v for k, v in w.items() if k.startswith('encoder/')}
    assert len(model) == 38 and sum(v.size for v in model.values()) == 245253
    assert w['encoder/CBHG/conv1d_1/conv1d/kernel'].shape == (3, 768, 40)
    assert w['encoder/CBHG/gru/bidirectional_rnn/fw/gru_cell/gates/kernel'].shape == (80, 80)
    # training-state scalars: lr = lr_start / (1 + decay * epoch)
    assert int(w['opt/epoch']) == 947 and int(w['opt/global_step']) == 136512
    lr = float(w['opt/learning_rate_start']) / (1.0 + float(w['opt/learning_rate_decay']) * 947)
    assert abs(float(w['opt/learning_rate']) - lr) < 1e-9
    assert w['opt/epoch'].shape == () and w['opt/epoch'].dtype == np.int32


def _reference_bundle(golden_dir, tmp_path, ck):
    """The reference's checkpoint `ck` rebuilt from tests/golden/reference_ckpt/<ck> (tools/make_golden.py): its
    TF-written .index verbatim, and its data blob re-assembled byte for byte -- every tensor at the offset TF's index
    gives it, checked against the blob's recorded size and SHA-256.  Returns the bundle prefix."""
    import glob
    import hashlib
    import shutil
    src = os.path.join(golden_dir, 'reference_ckpt', ck)
    meta = json.load(open(os.path.join(src, 'bundle.json')))
    dst = tmp_path / ck
    dst.mkdir()
    prefix = str(dst / meta['prefix'])
    shutil.copyfile(os.path.join(src, meta['prefix'] + '.index'), prefix + '.index')
    tensors = {}
    if meta['model_tensors_from']:
        tensors.update(tf_bundle.read_bundle(os.path.join(golden_dir, meta['model_tensors_from'], meta['prefix'])))
    for f in sorted(glob.glob(os.path.join(src, 'tensors_*.npz'))):
        tensors.update(np.load(f))
    blob = bytearray(meta['data_size'])
    for name, e in tf_bundle.list_bundle(prefix).items():
        raw = np.ascontiguousarray(tensors[name]).tobytes()
        assert len(raw) == e.size, name
        blob[e.offset:e.offset + e.size] = raw
    assert hashlib.sha256(blob).hexdigest() == meta['data_sha256']
    with open(prefix + '.data-00000-of-00001', 'wb') as f:
        f.write(blob)
    return prefix


def test_reference_checkpoints_readable(golden_dir, tmp_path):
    for ck, n in (('enc_14_ckpt', 109), ('enc_6_ckpt', None)):
        prefix = _reference_bundle(golden_dir, tmp_path, ck)
        w = tf_bundle.read_bundle(prefix, verify_crc=True)          # every tensor CRC-checked
        if n is not None:
            assert len(w) == n
    ref = os.path.join(golden_dir, 'reference_ckpt')
    assert tf_bundle.latest_checkpoint(os.path.join(ref, 'enc_14_ckpt')).endswith('encoder-136512')
    # enc_2_ckpt ships an index but no data blob (.MISSING_LARGE_BLOBS)
    with pytest.raises(Exception):
        tf_bundle.read_bundle(os.path.join(ref, 'enc_2_ckpt', 'encoder-136152'))


def test_writer_is_byte_compatible_with_tf(golden_dir, tmp_path):
    src = _reference_bundle(golden_dir, tmp_path, 'enc_14_ckpt')
    w = tf_bundle.read_bundle(src, verify_crc=False)
    dst = str(tmp_path / 'encoder-1')
    tf_bundle.write_bundle(dst, w)
    with open(src + '.data-00000-of-00001', 'rb') as a, open(dst + '.data-00000-of-00001', 'rb') as b:
        assert a.read() == b.read()                                  # same order, same packing
    assert tf_bundle.list_bundle(src) == tf_bundle.list_bundle(dst)  # same entry protos


def test_roundtrip_many_blocks(tmp_path):
    rng = np.random.RandomState(0)
    t = {'scope_%03d/sub/kernel' % i: rng.standard_normal((3, i + 1)).astype(np.float32) for i in range(300)}
    t['opt/global_step'] = np.array(7, dtype=np.int32)
    t['opt/flag'] = np.array([True, False])
    t['a/i64'] = np.arange(5, dtype=np.int64)
    prefix = str(tmp_path / 'm' / 'model-7')
    tf_bundle.write_bundle(prefix, t, block_size=512)                # forces many SSTable blocks
    r = tf_bundle.read_bundle(prefix)
    assert set(r) == set(t)
    for k in t:
        assert r[k].dtype == t[k].dtype and r[k].shape == t[k].shape and np.array_equal(r[k], t[k])
    tf_bundle.update_checkpoint_state(str(tmp_path / 'm'), 'model-7')
    assert tf_bundle.latest_checkpoint(str(tmp_path / 'm')) == prefix
    assert tf_bundle.latest_checkpoint(str(tmp_path)) is None


def test_corruption_detected(tmp_path):
    prefix = str(tmp_path / 'c-1')
    tf_bundle.write_bundle(prefix, {'x': np.arange(10, dtype=np.float32)})
    p = prefix + '.data-00000-of-00001'
    raw = bytearray(open(p, 'rb').read())
    raw[5] ^= 0x40
    open(p, 'wb').write(bytes(raw))
    with pytest.raises(ValueError):
        tf_bundle.read_bundle(prefix)
    assert tf_bundle.read_bundle(prefix, verify_crc=False)['x'].shape == (10,)
