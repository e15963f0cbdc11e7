"""numpy reference of the device's initial-phase generator (include/vc_hip.h, vc_phase_init): Philox4x32-10 (Salmon,
Moraes, Dror & Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the addressing
phase[f, k] = float32(pi) * ((x >> 8) * 2^-24), x = word e % 4 of the block with counter (e // 4, utt_id, 0, 0) and key
(seed & 0xFFFFFFFF, seed >> 32), e = f * n_bins + k.  Test infrastructure only."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def phase_ref(seed, utt_id, n_frames, n_bins):
    """float32 [n_frames, n_bins]: what vc_phase_init writes for the first n_frames rows of an utterance."""
    n = int(n_frames) * int(n_bins)
    blocks = (n + 3) // 4
    words = philox4x32_10((np.arange(blocks), np.uint32(int(utt_id) & 0xFFFFFFFF), 0, 0),
                          (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    x = np.stack(words, axis=1).reshape(-1)[:n]
    u = (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (np.float32(np.pi) * u).astype(np.float32).reshape(int(n_frames), int(n_bins))
