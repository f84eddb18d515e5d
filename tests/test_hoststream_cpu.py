"""CPU tests of the host-fed streams (spiht_amd/hoststream.py, csrc/hstream_ring.h): the ring's bookkeeping as a
stand-alone host program under the address and undefined-behaviour sanitizers, and the Python layer against a fake backend
with the same three calls -- input, submit, next -- so that order, short batches, refusals and close are checked without a
GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_program_under_sanitizers(tmp_path):
    """tests/native/hstream_ring_check.cpp: every order of input / submit / next for depth 2, 3 and 4 over 50 steps, busy on
    a full ring, the timeout's return path, reuse only after a result was taken, results in order.  A host program of its
    own: built with the host compiler and -fsanitize=address,undefined, run as a child process."""
    exe = str(tmp_path / "hstream_ring_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "hstream_ring_check.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hstream_ring_check ok" in r.stdout and "runtime error" not in r.stderr


def test_ring_header_has_no_hip():
    src = open(os.path.join(ROOT, "spiht_amd", "csrc", "hstream_ring.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "hip" not in code.lower() and "#include <stdint.h>" in code


# ---- the Python layer against a fake backend ----------------------------------------------------------------------------

class FakeBackend:
    """The three calls of a stream on the CPU, with the ring's rules: `depth` slots in ring order, busy when the next one is
    still in flight, results oldest first.  An encoder's "stream" of a picture is its first 1 + (sum mod 5) bytes and
    max_n = its first byte mod 31; a decoder's "picture" of a stream is filled with len(stream) + max_n."""

    def __init__(self, direction, store, B, depth, pic_shape, slot_bytes=64):
        from spiht_amd import hoststream as hs
        self.hs, self.direction, self.store, self.B, self.depth = hs, direction, np.dtype(store), B, depth
        self.pic_shape, self.slot_bytes = tuple(pic_shape), slot_bytes
        self.slots = [self._staging() for _ in range(depth)]
        self.results = [None] * depth
        self.issued = self.taken = 0
        self.handed = False
        self.closed = 0
        self.log = []

    def _staging(self):
        if self.direction == 0:
            return np.zeros((self.B,) + self.pic_shape, self.store)
        return (np.zeros(self.B * self.slot_bytes, np.uint8), np.zeros(self.B, np.uint32), np.zeros(self.B, np.uint8))

    def input(self):
        if not self.handed and self.issued - self.taken == self.depth:
            raise self.hs.StreamBusy("full")
        self.handed = True
        return self.slots[self.issued % self.depth]

    def submit(self, n, device_out=None):
        if not self.handed:
            raise self.hs.StreamBusy("full") if self.issued - self.taken == self.depth else ValueError("no input")
        i = self.issued % self.depth
        if self.direction == 0:
            pics = self.slots[i][:n]
            streams = [p.reshape(-1).view(np.uint8)[:1 + int(p.astype(np.float64).sum()) % 5].copy() for p in pics]
            self.results[i] = (np.concatenate(streams), np.array([len(s) for s in streams], np.uint32),
                               np.array([int(s[0]) % 31 for s in streams], np.uint8))
        else:
            _, lens, max_n = self.slots[i]
            out = np.zeros((n,) + self.pic_shape, self.store)
            for b in range(n):
                out[b] = int(lens[b]) + int(max_n[b])
            self.results[i] = out
        self.log.append(n)
        self.handed = False
        self.issued += 1

    def next(self, timeout_ms):
        if self.issued == self.taken:
            raise self.hs.StreamIdle("idle")
        out = self.results[self.taken % self.depth]
        self.taken += 1
        return out

    def close(self):
        self.closed += 1


def _fake_stream_of(p):
    b = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
    return b[:1 + int(p.astype(np.float64).sum()) % 5].tobytes(), int(b[0]) % 31


def _pictures(n, shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 250, shape).astype(dtype) for _ in range(n)]


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_encoder_run_keeps_order_and_takes_short_batches(depth):
    from spiht_amd import hoststream as hs
    B, shape = 3, (2, 4, 5)
    be = FakeBackend(0, np.uint8, B, depth, shape)
    enc = hs.StreamEncoder(*shape, dtype=np.uint8, batch=B, depth=depth, level=2, _backend=be)
    pics = _pictures(3 * 6 + 1, shape, np.uint8)
    batches = [np.stack(pics[i:i + B]) for i in range(0, len(pics), B)]   # 7 steps, the last with n = 1: more steps than slots
    got = list(enc.run(batches))
    assert [len(g) for g in got] == [3] * 6 + [1] and be.log == [3] * 6 + [1]
    flat = [r for g in got for r in g]
    for p, r in zip(pics, flat):
        data, mn = _fake_stream_of(p)
        assert (r.encoded_bytes, r.max_n, r.h, r.w, r.c, r.level) == (data, mn, 4, 5, 2, 2)
    assert enc.pending() == 0
    enc.close()
    enc.close()
    assert be.closed == 1
    with pytest.raises(ValueError):
        enc.input()


def test_encoder_calls_busy_idle_and_refusals():
    from spiht_amd import hoststream as hs
    B, shape = 2, (1, 3, 3)
    be = FakeBackend(0, np.float64, B, 2, shape)
    enc = hs.StreamEncoder(*shape, dtype=np.float64, batch=B, depth=2, _backend=be)
    with pytest.raises(hs.StreamIdle):
        enc.next(0)
    for k in range(2):
        enc.input()[:] = k + 1
        enc.submit(2)
    with pytest.raises(hs.StreamBusy):
        enc.input()
    with pytest.raises(hs.StreamBusy):
        enc.submit(1)
    assert enc.pending() == 2
    assert len(enc.next()) == 2
    enc.input()[:1] = 7
    for bad in (0, 3, -1):
        with pytest.raises(ValueError):
            enc.submit(bad)
    enc.submit(1)
    assert [len(enc.next()), len(enc.next())] == [2, 1]
    # what run() refuses, by the batch's index
    for bad in (np.zeros((3,) + shape), np.zeros((1, 1, 3, 4)), np.zeros(shape), np.zeros((1,) + shape, np.float32)):
        with pytest.raises(ValueError, match="batch 1"):
            list(enc.run([np.zeros((2,) + shape), bad]))
        while enc.pending():
            enc.next()
    for kw in (dict(depth=1), dict(depth=5), dict(batch=0)):
        with pytest.raises(ValueError):
            hs.StreamEncoder(*shape, _backend=be, **kw)
    with pytest.raises(TypeError):
        hs.StreamEncoder(*shape, dtype=np.int32, _backend=be)
    with pytest.raises(ValueError):
        hs.StreamEncoder(2, 3, 3, hs.SpihtSettings(color_model="IPT"), _backend=be)
    with pytest.raises(OverflowError):
        hs.StreamEncoder(*shape, max_bits=-1, _backend=be)


@pytest.mark.parametrize("dtype", [np.float64, np.uint8, np.uint16, np.float16, "bfloat16"])
def test_decoder_run_keeps_order(dtype):
    from spiht_amd import hoststream as hs
    from spiht_amd import EncodingResult
    B, depth, shape = 3, 2, (3, 4, 6)
    store = hs._element(dtype).storage
    be = FakeBackend(1, store, B, depth, shape)
    dec = hs.StreamDecoder(*shape, level=1, dtype=dtype, batch=B, depth=depth, _backend=be)
    res = [EncodingResult(bytes(range(1 + k % 9)), 4, 6, 3, k % 20, 1) for k in range(19)]
    lists = [res[i:i + B] for i in range(0, len(res), B)]
    got = list(dec.run(lists))
    assert [len(g) for g in got] == [3] * 6 + [1]
    flat = np.concatenate(got)
    assert flat.dtype == store and flat.shape == (19,) + shape
    assert [int(p.flat[0]) for p in flat] == [1 + k % 9 + k % 20 for k in range(19)]
    # the refusals: another geometry, a stream longer than the staging, too many streams
    other = EncodingResult(b"ab", 4, 7, 3, 5, 1)
    with pytest.raises(ValueError, match="stream 1 of batch 1"):
        list(dec.run([res[:2], [res[0], other]]))
    while dec.pending():
        dec.next()
    with pytest.raises(ValueError, match="bytes"):
        dec.put([EncodingResult(bytes(be.slot_bytes + 1), 4, 6, 3, 5, 1)])
    with pytest.raises(ValueError):
        dec.put(res[:4])
    with pytest.raises(ValueError):
        dec.put([])
    dec.close()
    dec.close()
    assert be.closed == 1


def test_conveniences_yield_one_per_input_in_order():
    from spiht_amd import hoststream as hs
    from spiht_amd import EncodingResult
    shape = (3, 5, 4)
    made = []

    def backend(direction, store):
        def make(c, H, W):
            made.append(FakeBackend(direction, store, 4, 3, (c, H, W)))
            return made[-1]
        return make

    for fn, dtype, kw in ((hs.encode_images, np.float64, {}), (hs.encode_images_u8, np.uint8, {}), (hs.encode_images_u16, np.uint16, {}),
                          (hs.encode_images_float, np.float32, {}), (hs.encode_images_float, np.uint16, dict(dtype="bfloat16"))):
        pics = _pictures(10, shape, dtype, seed=3)
        out = list(fn(iter(pics), None, 2, 100, batch=4, depth=3, _backend=backend(0, dtype), **kw))   # 4 + 4 + 2
        assert len(out) == 10 and made[-1].log == [4, 4, 2] and made[-1].closed == 1
        for p, r in zip(pics, out):
            assert (r.encoded_bytes, r.max_n) == _fake_stream_of(p) and (r.c, r.h, r.w, r.level) == (3, 5, 4, 2)
        assert list(fn([], _backend=backend(0, dtype), **kw)) == []
        # a picture of another shape: ValueError that names its index; the stream is closed all the same
        bad = pics[:5] + [np.zeros((3, 5, 5), dtype)] + pics[5:]
        with pytest.raises(ValueError, match="picture 5"):
            list(fn(bad, batch=4, _backend=backend(0, dtype), **kw))
        assert made[-1].closed == 1
        with pytest.raises(ValueError):
            list(fn([np.zeros(shape, np.int32)], _backend=backend(0, dtype), **kw))

    res = [EncodingResult(bytes(range(1 + k % 7)), 5, 4, 3, k, None) for k in range(9)]
    for fn, store, kw in ((hs.decode_images, np.float64, {}), (hs.decode_images_u8, np.uint8, {}), (hs.decode_images_u16, np.uint16, {}),
                          (hs.decode_images_float, np.float16, dict(dtype=np.float16))):
        out = list(fn(iter(res), None, batch=4, _backend=backend(1, store), **kw))
        assert len(out) == 9 and made[-1].log == [4, 4, 1] and made[-1].closed == 1
        assert all(o.shape == shape and o.dtype == store and int(o.flat[0]) == 1 + k % 7 + k for k, o in enumerate(out))
        assert list(fn([], _backend=backend(1, store), **kw)) == []
        bad = res[:6] + [EncodingResult(b"x", 5, 5, 3, 1, None)]
        with pytest.raises(ValueError, match="stream 6"):
            list(fn(bad, batch=4, _backend=backend(1, store), **kw))
        assert made[-1].closed == 1


def test_names_are_exported():
    import spiht
    import spiht_amd
    for name in ("StreamEncoder", "StreamDecoder", "StreamBusy", "StreamTimeout", "StreamIdle", "encode_images", "encode_images_u8",
                 "encode_images_u16", "encode_images_float", "decode_images", "decode_images_u8", "decode_images_u16",
                 "decode_images_float"):
        assert getattr(spiht, name) is getattr(spiht_amd, name)
    assert spiht.hoststream is spiht_amd.hoststream
    from spiht_amd import _lib
    L = _lib.lib()
    assert (_lib.ERR_BUSY, _lib.ERR_TIMEOUT, _lib.ERR_IDLE) == (11, 12, 13)
    texts = {L.spiht_strerror(s) for s in (11, 12, 13)}
    assert len(texts) == 3 and b"unknown status" not in texts
    # refused before any device is looked at
    import ctypes as C
    h = C.c_void_p()
    assert L.spiht_hstream_create(None, 0, 0, 1, 3, 1, 8, 8, 0, 0, -1, 50.0, None, 0, None, C.byref(h)) == _lib.ERR_ARG
    assert L.spiht_hstream_next(None, 0, None) == _lib.ERR_ARG and L.spiht_hstream_destroy(None) == _lib.OK
