"""The trajectory store's batch gather (k_store_scan, k_store_copy, csrc/ndp_store.inc) on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/host_drivers/store_gather.inc follows the library's source in main.hip and
runs every case by the kernels' schedule with the library's own __host__ __device__ functions (namespace ndp::store), every
buffer in an allocation of exactly its size -- the blob included, which the store does not pad: the copy's aligned reads
around an unaligned source range must narrow at the blob's two ends by themselves.  The streams are random bytes.  The
expected result is `pack_jpegs` of the selected streams plus numpy slices of the tables (tests/store_common.py), byte for
byte.  The sanitizers are on the host half of the stand-alone driver only; it runs as an ordinary child process.  No GPU
involved (the same cases on the GPU: tests/test_gpu_trajectory_store.py)."""
import numpy as np
import pytest

import host_driver
import store_common as C


@pytest.fixture(scope="module")
def driver():
    # a toolchain that cannot link the sanitizers' runtimes fails here: without them this file proves nothing
    return host_driver.build()


@pytest.fixture(scope="module")
def main_report(driver, tmp_path_factory):
    corpus = C.main_corpus()
    case_list = C.main_cases(corpus)
    return corpus, case_list, C.run_driver(driver, corpus, case_list, tmp_path_factory.mktemp("store_main"))


def test_the_corpus_is_what_the_cases_need():
    corpus = C.main_corpus()
    lengths = np.diff(corpus["offsets"])
    assert set(C.LENGTHS) <= set(lengths.tolist())
    assert C.LONG_STREAM >= 65537 and C.LONG_STREAM > C.CHUNK_BYTES and corpus["max_len"] == C.LONG_STREAM
    assert lengths[-1] > 0 and corpus["offsets"][-1] == corpus["blob"].size      # the last stream ends with the blob
    case_list = C.main_cases(corpus)
    assert [len(i) * t for _, i, _, t in case_list[-5:]] == [63, 64, 65, 1023, 1025]
    assert [(len(i), s, t) for _, i, s, t in case_list[:2]] == [(1, 0, 1), (3, 2, 5)]
    name, indices, seq_start, seq_length = case_list[2]
    assert list(indices) == [0, corpus["n"] - 1] and seq_start == 0 and seq_length == corpus["steps"]
    # every (source, destination) residue pair mod 16 occurs
    assert len(C.residue_pairs(corpus, case_list)) == 256
    # the long stream is selected, at an unaligned destination
    sel = C.selected(corpus, *case_list[3][1:])
    assert any(l == C.LONG_STREAM for _, l in sel)


def test_every_case_matches_pack_jpegs_and_the_table_slices(main_report):
    corpus, case_list, results = main_report
    for (name, indices, seq_start, seq_length), (got, changed) in zip(case_list, results):
        C.check(name, got, C.expected(corpus, indices, seq_start, seq_length))
        assert changed == 0, (name, "bytes past offsets[-1] were written", changed)


def test_out_of_range_indices_give_empty_streams_zero_rows_and_the_status(main_report):
    corpus, case_list, results = main_report
    by_name = {c[0]: r for c, r in zip(case_list, results)}
    (buffer, offsets, states, actions, goal, status), _ = by_name["out of range"]
    assert status == C.BAD_INDEX
    lengths = np.diff(offsets).reshape(6, 4)
    assert (lengths[[1, 3, 4]] == 0).all() and lengths[[0, 2, 5]].sum() == buffer.size
    assert not states[[1, 3, 4]].any() and not actions[[1, 3, 4]].any() and not goal[[1, 3, 4]].any()
    assert all(r[0][5] == 0 for n, r in by_name.items() if n != "out of range")


def test_a_store_of_one_frame_per_trajectory(driver, tmp_path):
    corpus = C.single_corpus()
    case_list = C.single_cases(corpus)
    assert (len(case_list[0][1]), corpus["steps"]) + case_list[0][2:] == (1, 1, 0, 1)
    for (name, indices, seq_start, seq_length), (got, changed) in zip(case_list, C.run_driver(driver, corpus, case_list, tmp_path)):
        C.check(name, got, C.expected(corpus, indices, seq_start, seq_length))
        assert changed == 0, name


def test_20480_short_streams(driver, tmp_path):
    corpus = C.tiny_corpus()
    case_list = C.tiny_cases(corpus)
    assert len(case_list[0][1]) * case_list[0][3] == 20480
    (got, changed), = C.run_driver(driver, corpus, case_list, tmp_path)
    C.check("20480", got, C.expected(corpus, *case_list[0][1:]))
    assert changed == 0
