"""The entry point reached and every argument of every C call behind the pixel-typed device methods of BatchCodec, Pipeline
and TiledCodec, held to the record tests/golden/pixel_calls.json (tests/pixel_call_cases.py: the cases, the recorder and how
an argument is written down).  The record was taken once, before the Python layer got one pixel element type; it is not
regenerated.  No device: the context is a stub, and creating a real one fails the test."""
import json

import pytest

import pixel_call_cases as P


@pytest.fixture(scope="module")
def golden():
    with open(P.GOLDEN) as f:
        return json.load(f)


@pytest.fixture
def no_context(monkeypatch):
    """any attempt to create a GPU context fails the test"""
    from spiht_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a context was created by a call on a stub context")
    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib.Context, "__init__", boom)


def test_the_record_holds_the_cases_of_the_table(golden):
    assert sorted(golden) == sorted(P.all_cases())
    assert all(golden[name] for name in golden)  # every case reaches the library


def test_every_element_reaches_its_own_entry_points(golden):
    """the record itself: seven elements, five suffixes, the kind behind the context"""
    def names(case):
        return [call[0] for call in golden[case]]
    for elem, sfx in (("f64", "f64"), ("f32", "f32"), ("u8", "u8"), ("u16", "u16"), ("float32", "flt"), ("float16", "flt"),
                      ("bfloat16", "flt")):
        coef = elem not in ("u8", "u16")
        assert names("LNone/encode/%s/st=None/coef=%s" % (elem, coef)) == ["spiht_encode_image_batch_" + sfx]
    for kind, elem in enumerate(("float32", "float16", "bfloat16"), 1):
        (name, args), = golden["L1/decode/%s/reduce=1/st=cl/rec=True/slot=64" % elem]
        assert name == "spiht_decode_image_reduced_batch_flt" and args[:2] == [0x10, kind] and args[-1] == 1
        assert args[-3][0] == "i64" and args[-3][2] == P.ES[elem]  # (channels-last: the channel stride is one sample)


@pytest.mark.parametrize("group", ["batch", "tiled"])
def test_calls_equal_the_record(group, golden, no_context):
    cases = P.batch_cases() if group == "batch" else P.tiled_cases()
    assert cases
    for name, case in cases.items():
        assert json.loads(json.dumps(case())) == golden[name], name
