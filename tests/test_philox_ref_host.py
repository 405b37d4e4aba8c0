"""CPU: the host restatement of the device noise stream (tests/philox_ref.py) against what is known without a GPU -- the
published Random123 known answers of philox4x32 with 10 rounds, the stream's layout as DESIGN.md section 3 defines it,
the independence of the 24 streams training uses (keys random_seed * 1000 + rank, offsets = successive G steps) and the
separation of the keys and offsets the callers choose.  tests/test_gpu_noise.py then holds the kernels to this file bit
for bit.

The statistical caps are conditions on a uniform i.i.d. stream, five standard deviations of each statistic at n = 2^18:
sd(mean) = sqrt(1 / (12 n)); sd(variance) = sqrt((mu4 - sigma^4) / n) = sqrt(1 / (180 n)) (mu4 = 1/80); a correlation of
standardised values has sd 1 / sqrt(n); a chi-square with 255 degrees of freedom has mean 255 and sd sqrt(510)."""
import contextlib
import glob
import os

import numpy as np
import pytest
import torch

import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's kat_vectors, philox4x32 with 10 rounds: counter, key, result
KNOWN_ANSWERS = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _hex(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter,key,result", KNOWN_ANSWERS)
def test_published_known_answers(counter, key, result):
    got = P.philox4x32_10(_hex(counter), _hex(key))
    assert got.dtype == np.uint64 and got.tolist() == _hex(result)


def test_known_answers_vectorised_over_counters():
    counters = np.array([_hex(c) for c, _, _ in KNOWN_ANSWERS], np.uint64)
    keys = np.array([_hex(k) for _, k, _ in KNOWN_ANSWERS], np.uint64)
    assert P.philox4x32_10(counters, keys).tolist() == [_hex(r) for _, _, r in KNOWN_ANSWERS]
    # one key against many counters
    same_key = P.philox4x32_10(counters, keys[2])
    assert same_key[2].tolist() == _hex(KNOWN_ANSWERS[2][2]) and same_key[0].tolist() != _hex(KNOWN_ANSWERS[0][2])
    # nine rounds are another function
    assert P.philox4x32_10(counters[2], keys[2], rounds=9).tolist() != _hex(KNOWN_ANSWERS[2][2])


# ------------------------------------------------------------------------------------------------ the stream's layout
def test_uniform_is_word_e_and_3_of_block_e_shift_2():
    seed, offset, n = (7 << 32) | 0x89ABCDEF, 5, 64
    u = P.uniform(seed, offset, n)
    assert u.dtype == np.float32 and u.shape == (n,)
    for j in range(n // 4):
        block = P.philox4x32_10([j, 0, offset, 0x6e647021], [0x89ABCDEF, 7])
        for w in range(4):
            assert u[4 * j + w] == np.float32((int(block[w]) >> 8) * 2.0 ** -24), (j, w)
    # each of the counter and key words matters: offset, the constant word's place, the key's high word
    assert not np.array_equal(u, P.uniform(seed, offset + 1, n))
    assert not np.array_equal(u, P.uniform(seed & 0xFFFFFFFF, offset, n))
    assert not np.array_equal(u, P.uniform(seed + 1, offset, n))


def test_values_are_multiples_of_2_to_the_minus_24_in_the_unit_interval():
    u = P.uniform(123, 0, 1 << 16).astype(np.float64)
    assert (u >= 0).all() and (u < 1).all()
    scaled = u * 2.0 ** 24
    assert np.array_equal(scaled, np.floor(scaled))
    assert np.array_equal(P.words(123, 0, 1 << 16) >> np.uint64(8), scaled.astype(np.uint64))


def test_start_is_a_slice_of_the_stream_from_zero():
    whole = P.uniform(99, 2, 1037)
    for start, n in ((0, 1), (1, 1), (3, 2), (4, 4), (5, 9), (255, 3), (1030, 7), (1036, 1)):
        assert np.array_equal(P.uniform(99, 2, n, start=start), whole[start:start + n]), (start, n)


def test_offset_none_is_zero_and_a_negative_offset_is_its_uint32():
    assert np.array_equal(P.uniform(5, None, 33), P.uniform(5, 0, 33))
    assert np.array_equal(P.uniform(5, -1, 33), P.uniform(5, 0xFFFFFFFF, 33))
    assert not np.array_equal(P.uniform(5, -1, 33), P.uniform(5, 0, 33))
    assert np.array_equal(P.uniform(2 ** 64 - 1, 1, 8), P.uniform(-1, 1, 8))          # the seed is a uint64


def test_a_block_index_above_2_to_the_32_reaches_the_second_counter_word():
    start = 1 << 34                                                   # block 2^32: counter (0, 1, offset, word)
    u = P.uniform(11, 3, 6, start=start + 1)
    first = P.philox4x32_10([0, 1, 3, 0x6e647021], [11, 0])
    second = P.philox4x32_10([1, 1, 3, 0x6e647021], [11, 0])
    want = [(int(w) >> 8) * 2.0 ** -24 for w in list(first[1:]) + list(second[:3])]
    assert u.tolist() == want
    assert not np.array_equal(u, P.uniform(11, 3, 6, start=1))          # block 0 is another block
    # the last block below the carry
    below = P.uniform(11, 3, 4, start=start - 4)
    want = P.philox4x32_10([0xFFFFFFFF, 0, 3, 0x6e647021], [11, 0])
    assert below.tolist() == [(int(w) >> 8) * 2.0 ** -24 for w in want]


# ------------------------------------------------------------------------------------------------ stream independence
N = 1 << 18
RANDOM_SEED, RANKS, OFFSETS = 5, range(8), (0, 1, 2)


@pytest.fixture(scope="module")
def streams():
    """{(key, offset): float64 [N]} for the 24 streams of an 8-rank run's first three G steps."""
    return {(RANDOM_SEED * 1000 + r, off): P.uniform(RANDOM_SEED * 1000 + r, off, N).astype(np.float64)
            for r in RANKS for off in OFFSETS}


def _standardised(u):
    return (u - 0.5) * np.sqrt(12.0)


def test_each_training_stream_is_uniform_and_uncorrelated_with_itself(streams):
    """Measured (the streams are fixed numbers, so these do not move): as a share of the cap, mean 0.29, variance 0.81
    (key 5002 at offset 0, -4.0 standard deviations; the next largest of the 24 is 0.32), autocorrelation 0.48;
    chi-square 212 .. 284 against the cap of 368."""
    assert len(streams) == 24
    worst = {"mean": 0.0, "var": 0.0, "autocorr": 0.0, "chi2": 0.0}
    for name, u in streams.items():
        mean, var = abs(u.mean() - 0.5), abs(u.var() - 1.0 / 12.0)
        assert mean <= 5 * np.sqrt(1.0 / (12 * N)), (name, mean)
        assert var <= 5 * np.sqrt(1.0 / (180 * N)), (name, var)
        z = _standardised(u)
        for lag in range(1, 9):
            c = abs(np.mean(z[:-lag] * z[lag:]))
            assert c <= 5 / np.sqrt(N), (name, lag, c)
            worst["autocorr"] = max(worst["autocorr"], c * np.sqrt(N) / 5)
        counts = np.bincount((u * 256).astype(np.int64), minlength=256)
        assert counts.size == 256
        chi2 = float(((counts - N / 256.0) ** 2).sum() / (N / 256.0))
        assert chi2 <= 255 + 5 * np.sqrt(510.0), (name, chi2)
        worst["mean"] = max(worst["mean"], mean / (5 * np.sqrt(1.0 / (12 * N))))
        worst["var"] = max(worst["var"], var / (5 * np.sqrt(1.0 / (180 * N))))
        worst["chi2"] = max(worst["chi2"], chi2)
    print("worst over the 24 streams, as a share of the cap: mean %.2f, variance %.2f, autocorrelation %.2f; "
          "largest chi-square %.1f (cap %.1f)" % (worst["mean"], worst["var"], worst["autocorr"], worst["chi2"],
                                                  255 + 5 * np.sqrt(510.0)))


def test_training_streams_are_uncorrelated_with_each_other_and_share_no_prefix(streams):
    names = list(streams)
    z = np.stack([_standardised(streams[n]) for n in names])
    corr = z @ z.T / N
    worst = 0.0
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            assert abs(corr[i, j]) <= 5 / np.sqrt(N), (names[i], names[j], corr[i, j])
            worst = max(worst, abs(corr[i, j]))
    print("largest cross-correlation of the 276 pairs: %.2f of the cap" % (worst * np.sqrt(N) / 5))
    heads = {streams[n][:16].tobytes() for n in names}
    assert len(heads) == 24


# ------------------------------------------------------------------------------------------------ who uses which key
def _committed_random_seeds():
    import yaml
    seeds = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "config", "*.yaml"))):
        with open(path) as f:
            cfg = yaml.safe_load(f)
        if isinstance(cfg, dict) and "random_seed" in cfg:
            seeds.add(int(cfg["random_seed"]))
    return seeds


def test_the_validation_key_is_apart_from_every_trainer_key():
    from ndivplanning_amd import train_gan
    seeds = _committed_random_seeds()
    assert seeds, "no committed config states a random_seed"
    trainer_keys = {s * 1000 + rank for s in seeds for rank in range(1000)}
    for s in seeds:
        assert train_gan.VAL_NOISE_SEED + s not in trainer_keys
    # ranks of one run never share a key, and runs with different seeds do not either while rank < 1000
    assert len(trainer_keys) == 1000 * len(seeds)
    assert train_gan.VAL_NOISE_SEED > 1000 * max(seeds) + 999 and train_gan.VAL_NOISE_SEED + max(seeds) < 2 ** 64


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_eval_models_normal_reads_offset_one_and_uniform_offset_zero(monkeypatch):
    """EvalModels.uniform passes no offset word (the kernels read that as 0), EvalModels.normal a word holding 1: the
    planner's proposals and the refinement's normal draws of one seed are different streams."""
    from ndivplanning_amd import _capi, evaluation as E
    monkeypatch.setattr(_capi, "on_device", lambda t: contextlib.nullcontext())
    monkeypatch.setattr(_capi, "stream_ptr", lambda device=None: None)
    models = E.EvalModels.__new__(E.EvalModels)
    models.lib, models.device = _RecordingLib(), torch.device("cpu")
    models.uniform(12, 77)
    models.normal(12, 2 ** 64 + 77)
    (name_u, args_u), (name_n, args_n) = models.lib.calls
    assert name_u == "ndp_uniform_noise" and name_n == "ndp_normal_noise"
    assert args_u[1:4] == (12, 77, None)
    assert args_n[1:3] == (12, 77)                                     # the seed is taken modulo 2^64
    assert args_n[3].value == models._normal_offset.data_ptr()
    assert models._normal_offset.dtype == torch.int32 and models._normal_offset.tolist() == [1]
