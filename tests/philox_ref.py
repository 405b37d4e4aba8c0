"""The device noise stream on the host, in plain numpy with uint64 arithmetic ("The noise stream").
Written from the definition of Philox-4x32 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC 2011) and pinned by the Random123 known answers (tests/test_philox_ref_host.py), not from the kernels: the GPU tests
hold `ndp_uniform_noise`, `ndp_normal_noise` and the draws inside the GAN step to it (tests/test_gpu_noise.py).

Philox-4x32, one round on the counter (c0, c1, c2, c3) with the round key (k0, k1):
    hi0 : lo0 = M0 * c0,  hi1 : lo1 = M1 * c2            (32 x 32 -> 64 bit products)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
Ten rounds; after every round but the last the key is bumped by the Weyl constants (W0, W1), modulo 2^32.

The stream (seed, offset): element e is word e & 3 of the block e >> 2, whose counter is (block low 32, block high 32,
offset as uint32, 0x6e647021) under the key (seed low 32, seed high 32); the value is (word >> 8) * 2^-24, a multiple
of 2^-24 in [0, 1).  The normals are `plan_common.box_muller` of these uniforms."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57         # the multipliers of Philox-4x32
W0, W1 = 0x9E3779B9, 0xBB67AE85         # the key schedule: golden ratio and sqrt(3) - 1, as 32-bit fractions
STREAM_WORD = 0x6e647021                # the fourth counter word of every block of the noise stream
_LOW = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def philox4x32_10(counter, key, rounds=10):
    """counter [..., 4], key [..., 2] (broadcast against each other), words below 2^32 -> the 4 output words [..., 4] as
    uint64 holding 32-bit values."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & _LOW, (k1 + np.uint64(W1)) & _LOW
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2             # below 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> _SH) ^ c1 ^ k0, p1 & _LOW, (p0 >> _SH) ^ c3 ^ k1, p0 & _LOW
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def words(seed, offset, n, start=0):
    """The 32-bit words of elements start .. start + n - 1 of the stream (seed, offset), as uint64 [n]."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    off = (0 if offset is None else int(offset)) & 0xFFFFFFFF
    start, n = int(start), int(n)
    first, last = start >> 2, (start + n - 1) >> 2
    blocks = np.arange(first, last + 1, dtype=np.uint64)
    counter = np.empty((blocks.size, 4), np.uint64)
    counter[:, 0], counter[:, 1] = blocks & _LOW, blocks >> _SH
    counter[:, 2], counter[:, 3] = off, STREAM_WORD
    out = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    lead = start - 4 * first
    return out.reshape(-1)[lead:lead + n]


def uniform(seed, offset, n, start=0):
    """float32 [n]: elements start .. start + n - 1 of the stream (seed, offset); offset None is 0, a negative offset its
    two's complement as uint32."""
    w = words(seed, offset, n, start) >> np.uint64(8)
    return (w.astype(np.float64) * 2.0 ** -24).astype(np.float32)           # 24 bits: exact in float32
