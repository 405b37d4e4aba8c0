"""The encoder corpus tests/golden/jpeg_encode_case.npz (made by tests/golden/make_golden_jpeg_encode.py): its streams are
this machine's PIL's -- the pin against a Pillow change, as tests/test_jpeg_core_host.py and the resize fixture have one
-- and it still meets its class conditions (a ZRL symbol, a stuffed 0xFF, a final padded byte of 0xFF, a stream without
padding, an all-EOB frame, a DC category of 10, an entropy segment above 20,000 bytes).  No GPU involved."""
import io

import numpy as np
import pytest

import jpeg_core_host as H
import jpeg_enc_core_host as E
from conftest import load_golden


@pytest.fixture(scope="module")
def corpus():
    return load_golden("jpeg_encode_case")


def test_the_committed_corpus_meets_its_class_conditions(corpus):
    E.check_classes(corpus)
    frames = E.corpus_frames(corpus)
    assert frames.shape == (len(corpus["names"]), 128, 128, 3)
    assert not frames[list(corpus["names"]).index("black")].any()


def test_fixture_streams_are_this_machine_s_pil(corpus):
    Image = pytest.importorskip("PIL.Image")
    features = pytest.importorskip("PIL.features")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this PIL is not built on libjpeg-turbo")
    frames = E.corpus_frames(corpus)
    for i, s in enumerate(E.corpus_streams(corpus)):
        assert E.pil_encode(frames[i]) == s, corpus["names"][i]
        assert np.array_equal(H.digest(np.array(Image.open(io.BytesIO(s)))), corpus["digest"][i]), corpus["names"][i]
    for j, frame in zip(corpus["env_index"], E.env_frames()):
        small = np.array(Image.fromarray(frame).resize((128, 128), Image.LANCZOS))
        assert np.array_equal(small, frames[j]), corpus["names"][j]
