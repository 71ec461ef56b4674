"""numpy restatement of the library's counter-based normal generator (rald_amd/csrc/rng.hip), shared by the sampler-churn tests.

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key
increments 0x9E3779B9 / 0xBB67AE85.  key = (seed mod 2^32, tag), counter = (e4, step, 0, 0) with e4 the index of the 4-element group;
Box-Muller on the word pairs (x0, x1) and (x2, x3): u1 = ((x >> 8) + 1) * 2^-24, u2 = (y >> 8) * 2^-24, r = sqrt(-2 ln u1),
(r cos(2 pi u2), r sin(2 pi u2)) - evaluated here in float64."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (values below 2^32, broadcastable) -> uint32 [..., 4]."""
    counter, key = np.asarray(counter, np.uint64), np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def normals(seeds, n_per_sample, tag, step):
    """float64 [B, n_per_sample]: what rald_op_philox_normal computes in fp32."""
    assert n_per_sample % 4 == 0
    seeds = np.asarray([int(s) % (1 << 32) for s in seeds], np.uint64)
    n4 = n_per_sample // 4
    counter = np.zeros((len(seeds), n4, 4), np.uint64)
    counter[..., 0] = np.arange(n4, dtype=np.uint64)[None, :]
    counter[..., 1] = step
    key = np.zeros((len(seeds), 1, 2), np.uint64)
    key[:, 0, 0] = seeds
    key[:, 0, 1] = tag
    w = philox4x32_10(counter, key).astype(np.float64)                  # [B, n4, 4]
    out = np.empty((len(seeds), n4, 4), np.float64)
    for a in (0, 2):
        u1 = (np.floor(w[..., a] / 256.0) + 1.0) * 2.0 ** -24           # (x >> 8) + 1
        u2 = np.floor(w[..., a + 1] / 256.0) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[..., a] = r * np.cos(2.0 * np.pi * u2)
        out[..., a + 1] = r * np.sin(2.0 * np.pi * u2)
    return out.reshape(len(seeds), n_per_sample)
