"""Host-fed streams: batches of host pictures encoded, or batches of streams decoded, with the transfers overlapped.

The reference's interface is host arrays in and host arrays out, one picture per call (spiht_wrapper.encode_image /
decode_image).  BatchCodec's host calls take a batch, but upload it, code it, download it and wait, one batch after the
other on one queue.  A stream (include/spiht_hip.h: spiht_hstream_*, csrc/hoststream.cpp) keeps a ring of `depth` steps in
flight over three queues -- step i+1's upload, step i's coding and step i-1's download run at the same time -- with
page-locked staging on both sides; the coding is the batched entry point of the pixel type, so the results are those of the
single-picture calls, bit for bit.

    enc = StreamEncoder(3, 1080, 1920, settings, level=None, max_bits=1036800, dtype=np.uint8, batch=32)
    for results in enc.run(batches):        # batches: arrays [n <= 32, 3, 1080, 1920]; results: n EncodingResults
        ...
    for r in encode_images_u8(pictures, settings, None, 1036800):   # any iterable of equally shaped pictures
        ...

The three calls underneath -- input() (the page-locked staging of the next step, to be filled in place), submit(n),
next(timeout) -- never wait without bound: input / submit raise StreamBusy when the ring is full, next raises StreamTimeout
after `timeout` seconds and may be called again.

The arrays input(), next(raw=True) and next(copy=False) return are VIEWS of the stream's page-locked staging: they hold no
reference to the stream, are valid until input() hands their slot out again, and must not be touched after close(), which gives
the memory back.  Everything else these calls return is a copy.
"""
import ctypes as C

import numpy as np

from . import _lib, color_models, px
from .spiht_wrapper import EncodingResult, SpihtSettings, _geometry, _mults_arg, _wavelet_mode_ids

ENCODE, DECODE = _lib.ENUMS["SPIHT_HS_ENCODE"], _lib.ENUMS["SPIHT_HS_DECODE"]
DEFAULT_TIMEOUT = 30.0  # seconds a generator waits for one step before it gives up (StreamTimeout)


class StreamBusy(RuntimeError):
    """input() / submit() with every slot of the ring in flight (SPIHT_ERR_BUSY): take a result with next() first"""


class StreamTimeout(TimeoutError):
    """next(): the oldest step did not complete within the time given (SPIHT_ERR_TIMEOUT); the stream is as it was"""


class StreamIdle(RuntimeError):
    """next() with nothing submitted (SPIHT_ERR_IDLE)"""


def _check(status):
    if status == _lib.ERR_BUSY:
        raise StreamBusy("every slot of the stream's ring is in flight")
    if status == _lib.ERR_TIMEOUT:
        raise StreamTimeout("the step did not complete within the time given")
    if status == _lib.ERR_IDLE:
        raise StreamIdle("nothing is submitted")
    _lib.check(status)


def _element(dtype):
    """dtype as BatchCodec's pixel calls name it -> its px.Elem: float64, uint8 and uint16 by dtype, everything else a float
    kind (np.float32 is the kind here, not the codec's own single-precision pixels)"""
    d = None
    if type(dtype).__module__.split(".")[0] != "torch" and dtype is not None:
        try:
            d = np.dtype(dtype)
        except TypeError:   # ("bfloat16": numpy has no such type)
            d = None
    for elem in (px.F64, px.U8, px.U16):
        if d is not None and d == elem.storage:  # (a dtype compares equal to None as to float64)
            return elem
    return px.of_kind(dtype)


def _view(ptr, nbytes, dtype, shape):
    """the memory at ptr as a numpy array (no copy; the stream owns the memory)"""
    buf = (C.c_char * int(nbytes)).from_address(int(ptr))
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)


class _NativeBackend:
    """spiht_hstream behind the three calls; what a fake backend of the tests stands in for"""

    def __init__(self, direction, elem, B, depth, c, H, W, wid, mid, lv, q, mults_p, max_bits, ctx, channels_last=False):
        self.L = _lib.lib()
        self.direction, self.store, self.B, self.depth, self.c = direction, elem.storage, int(B), int(depth), int(c)
        self.channels_last = bool(channels_last)
        h = C.c_void_p()
        st = None
        if self.channels_last:   # the view [B, c, H, W] of dense [B, H, W, c] pictures, in bytes
            st = np.ascontiguousarray(elem.channels_last_strides((self.B, self.c, int(H), int(W))), dtype=np.int64)
        _check(self.L.spiht_hstream_create(ctx.handle, direction, elem.stream_id, self.B, self.depth, self.c, int(H), int(W), wid, mid, lv,
                                           float(q), mults_p, int(max_bits), C.c_void_p(st.ctypes.data) if st is not None else None,
                                           C.byref(h)))
        self.handle = h
        sb, pb, rh, rw = C.c_uint64(), C.c_uint64(), C.c_int64(), C.c_int64()
        _check(self.L.spiht_hstream_info(h, C.byref(sb), C.byref(pb), C.byref(rh), C.byref(rw)))
        self.slot_bytes, self.pic_bytes = int(sb.value), int(pb.value)
        # one staged picture (a float64 decoder's: uncropped)
        self.pic_shape = (int(rh.value), int(rw.value), self.c) if self.channels_last else (self.c, int(rh.value), int(rw.value))

    def input(self):
        if self.direction == ENCODE:
            p = C.c_void_p()
            _check(self.L.spiht_hstream_input(self.handle, C.byref(p)))
            return _view(p.value, self.pic_bytes, self.store, (self.B,) + self.pic_shape)
        pk, ln, mn = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self.L.spiht_hstream_decode_input(self.handle, C.byref(pk), C.byref(ln), C.byref(mn)))
        return (_view(pk.value, self.B * self.slot_bytes, np.uint8, (self.B * self.slot_bytes,)),
                _view(ln.value, 4 * self.B, np.uint32, (self.B,)), _view(mn.value, self.B, np.uint8, (self.B,)))

    def submit(self, n, device_out=None):
        _check(self.L.spiht_hstream_submit(self.handle, int(n), C.c_void_p(device_out) if device_out else None))

    def next(self, timeout_ms):
        r = _lib.HStreamResult()
        _check(self.L.spiht_hstream_next(self.handle, int(timeout_ms), C.byref(r)))
        n = int(r.n)
        if self.direction == ENCODE:
            total = int(r.nbytes)
            data = _view(r.bytes, total, np.uint8, (total,)) if total else np.zeros(0, np.uint8)
            return data, _view(r.lens, 4 * n, np.uint32, (n,)), _view(r.max_n, n, np.uint8, (n,))
        if not r.pictures:
            return None
        return _view(r.pictures, int(r.nbytes), self.store, (n,) + self.pic_shape)

    def pending(self):
        k = C.c_int()
        _check(self.L.spiht_hstream_pending(self.handle, C.byref(k)))
        return int(k.value)

    def close(self):
        if self.handle:
            h, self.handle = self.handle, None
            _check(self.L.spiht_hstream_destroy(h))


class _Stream:
    """what StreamEncoder and StreamDecoder share: the settings, the backend and its life"""

    def __init__(self, direction, c, H, W, settings, level, max_bits, dtype, batch, depth, ctx, backend, channels_last=False):
        self.settings = settings if settings is not None else SpihtSettings()
        self.c, self.H, self.W, self.level = int(c), int(H), int(W), level
        self.batch, self.depth = int(batch), int(depth)
        if self.batch < 1:
            raise ValueError("batch must be at least 1")
        if not 2 <= self.depth <= 4:
            raise ValueError("depth must be 2, 3 or 4")
        self.elem = _element(dtype)
        self.store = self.elem.storage
        self.channels_last = bool(channels_last)
        if self.channels_last and not self.elem.view:
            raise ValueError("float64 pictures are dense (c, H, W); channels_last is for the integer and float kinds")
        self.pic_shape = (self.H, self.W, self.c) if self.channels_last else (self.c, self.H, self.W)
        cm = self.settings.color_model
        if cm is not None:
            if cm not in color_models.SUPPORTED_MODELS:
                raise ValueError(f'{cm} is not a supported color model. Supported models are {color_models.SUPPORTED_MODELS}')
            if self.c != 3:
                raise ValueError("colour conversion needs 3 channels")
        self._closed = False
        self._pending = 0
        if backend is not None:
            self.ctx, self._be = ctx, backend
            return
        wid, mid = _wavelet_mode_ids(self.settings)
        self.geom = _geometry(self.H, self.W, wid, level, mid)
        self._mults, mults_p = _mults_arg(self.settings.per_channel_quant_scales, self.c)
        self.ctx = ctx if ctx is not None else _lib.default_context()
        self._be = _NativeBackend(direction, self.elem, self.batch, self.depth, self.c, self.H, self.W, wid, mid,
                                  -1 if level is None else int(level), self.settings.quantization_scale, mults_p, max_bits, self.ctx,
                                  self.channels_last)

    def _color(self):
        # the colour model is the context's at the moment of the submit, which queues the whole step and returns
        return color_models.fused(self.ctx, self.settings.color_model) if self.ctx is not None else _NoColor()

    def _live(self):
        if self._closed:
            raise ValueError("the stream is closed")

    def input(self):
        """the page-locked staging of the next step, to be filled in place; StreamBusy when every slot is in flight"""
        self._live()
        return self._be.input()

    def pending(self):
        """steps submitted and not yet taken"""
        return self._pending

    def _next(self, timeout):
        self._live()
        out = self._be.next(max(0, int(round(float(timeout) * 1000.0))))
        self._pending -= 1
        return out

    def close(self):
        """waits (bounded) for what is queued and frees the stream; a second call does nothing"""
        if not self._closed:
            self._closed = True
            self._be.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _NoColor:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class StreamEncoder(_Stream):
    """Encodes batches of up to `batch` host pictures [n, c, H, W] of `dtype` -- float64, uint8, uint16, or a float kind
    of floatpx.kind_arg (float32, float16, "bfloat16": uint16 bit patterns) -- with the meaning of encode_image,
    encode_image_u8, encode_image_u16, encode_image_float: settings (colour model and channel scales included), level,
    max_bits.  `depth` (2 .. 4) steps are in flight at once.  channels_last (not float64): the pictures are [n, H, W, c], as
    the single-picture calls take them with channels_last -- the staging is laid out that way and the device reads it by
    strides."""

    def __init__(self, c, H, W, settings=None, level=None, max_bits=None, dtype=np.float64, batch=32, depth=3, ctx=None,
                 channels_last=False, _backend=None):
        mb = 99999999999999999 if max_bits is None else int(max_bits)
        if mb < 0:
            raise OverflowError("can't convert negative int to unsigned")
        super().__init__(ENCODE, c, H, W, settings, level, mb, dtype, batch, depth, ctx, _backend, channels_last)

    def submit(self, n):
        """queues pictures [0, n) of the staging input() gave; returns at once"""
        self._live()
        n = int(n)
        if not 1 <= n <= self.batch:
            raise ValueError("a step takes 1 .. %d pictures, not %d" % (self.batch, n))
        with self._color():
            self._be.submit(n)
        self._pending += 1

    def next(self, timeout=DEFAULT_TIMEOUT, raw=False):
        """the OLDEST submitted step -> its EncodingResults (their bytes are copies: they outlive the slot).  raw=True:
        (bytes, lens, max_n) as views of the page-locked staging -- the streams one behind the other, their lengths, their
        start planes -- valid until input() hands that slot out again"""
        data, lens, max_n = self._next(timeout)
        if raw:
            return data, lens, max_n
        out, o = [], 0
        for b in range(len(lens)):
            k = int(lens[b])
            out.append(EncodingResult(data[o:o + k].tobytes(), self.H, self.W, self.c, int(max_n[b]), self.level))
            o += k
        return out

    def _batch_arg(self, pictures, index):
        a = np.asarray(pictures)
        if a.ndim != 4 or a.shape[1:] != self.pic_shape or not 1 <= a.shape[0] <= self.batch:
            raise ValueError("batch %d has shape %s; the stream takes [1 .. %d, %d, %d, %d]"
                             % ((index, a.shape, self.batch) + self.pic_shape))
        if a.dtype.newbyteorder("=") != self.store:
            raise ValueError("batch %d is %s; the stream's pictures are %s" % (index, a.dtype, self.store.name))
        return a

    def run(self, batches, timeout=DEFAULT_TIMEOUT):
        """batches: an iterable of arrays [n <= batch, c, H, W] -> yields, per batch and in order, the list of its
        EncodingResults; up to `depth` batches are in flight while the caller works on a result"""
        for i, pictures in enumerate(batches):
            a = self._batch_arg(pictures, i)
            if self._pending == self.depth:
                yield self.next(timeout)
            self.input()[:a.shape[0]] = a
            self.submit(a.shape[0])
        while self._pending:
            yield self.next(timeout)


class StreamDecoder(_Stream):
    """Decodes batches of up to `batch` streams of one geometry into pictures of `dtype` with the meaning of
    decode_image (float64: [n, c, H', W'], uncropped as decode_image returns them), decode_image_u8, decode_image_u16,
    decode_image_float ([n, c, H, W]).  A stream does not record the pixel type it came from: any stream decodes into
    any type.  max_bytes: the longest stream it takes (None: the bound of the geometry); it sizes the staging.
    channels_last (not float64): the pictures come out as [n, H, W, c] -- on the host and at a device destination alike."""

    def __init__(self, c, H, W, settings=None, level=None, dtype=np.float64, batch=32, depth=3, ctx=None, max_bytes=None,
                 channels_last=False, _backend=None):
        if max_bytes is not None and int(max_bytes) < 1:
            raise ValueError("max_bytes must be at least 1")
        super().__init__(DECODE, c, H, W, settings, level, 0 if max_bytes is None else 8 * int(max_bytes), dtype, batch, depth,
                         ctx, _backend, channels_last)

    def _check_results(self, results, index):
        results = list(results)
        if not 1 <= len(results) <= self.batch:
            raise ValueError("batch %d has %d streams; the stream takes 1 .. %d" % (index, len(results), self.batch))
        for j, r in enumerate(results):
            if (r.c, r.h, r.w, r.level) != (self.c, self.H, self.W, self.level):
                raise ValueError("stream %d of batch %d is of a picture (c, h, w, level) = %s; the stream's are %s"
                                 % (j, index, (r.c, r.h, r.w, r.level), (self.c, self.H, self.W, self.level)))
            if len(r.encoded_bytes) > self._be.slot_bytes:
                raise ValueError("stream %d of batch %d has %d bytes; the stream takes %d at most"
                                 % (j, index, len(r.encoded_bytes), self._be.slot_bytes))
            if not 0 <= int(r.max_n) <= 255:
                raise OverflowError("out of range integral type conversion attempted")
        return results

    def submit(self, n, device_out=None):
        """queues streams [0, n) of the staging input() gave -- (packed bytes, lens, max_n): the streams one behind the
        other -- and returns at once.  device_out: a device pointer (int) the pictures go to instead of the host"""
        self._live()
        n = int(n)
        if not 1 <= n <= self.batch:
            raise ValueError("a step takes 1 .. %d streams, not %d" % (self.batch, n))
        with self._color():
            self._be.submit(n, device_out)
        self._pending += 1

    def put(self, results, device_out=None, index=0):
        """input() + the streams of `results` into it + submit()"""
        results = self._check_results(results, index)
        packed, lens, max_n = self.input()
        o = 0
        for b, r in enumerate(results):
            k = len(r.encoded_bytes)
            packed[o:o + k] = np.frombuffer(r.encoded_bytes, np.uint8)
            lens[b], max_n[b] = k, int(r.max_n)
            o += k
        self.submit(len(results), device_out)

    def next(self, timeout=DEFAULT_TIMEOUT, copy=True):
        """the OLDEST submitted step -> its pictures [n, ...] (None: they went to the device).  copy=False: a view of the
        page-locked staging, valid until input() hands that slot out again"""
        out = self._next(timeout)
        return out if out is None or not copy else np.array(out)

    def run(self, lists_of_results, timeout=DEFAULT_TIMEOUT):
        """lists_of_results: an iterable of lists of up to `batch` EncodingResults -> yields, per list and in order, the
        array of its pictures"""
        for i, results in enumerate(lists_of_results):
            results = self._check_results(results, i)
            if self._pending == self.depth:
                yield self.next(timeout)
            self.put(results, index=i)
        while self._pending:
            yield self.next(timeout)


# ---- conveniences: one picture or one stream at a time, any iterable of them ----------------------------------------------

def _batched(items, batch):
    group = []
    for x in items:
        group.append(x)
        if len(group) == batch:
            yield group
            group = []
    if group:
        yield group


def _encode_stream(images, settings, level, max_bits, batch, depth, ctx, dtype, name, _backend):
    """the generator behind encode_images*: the first picture says the shape; every picture is written straight into the
    staging of the step it belongs to (one copy); the stream is closed when the generator ends"""
    store = _element(dtype).storage
    enc, buf, n = None, None, 0
    try:
        for i, im in enumerate(images):
            a = np.asarray(im)
            if enc is None:
                if a.ndim != 3:
                    raise ValueError("picture 0: image ndim must be 3: c,h,w")
                if a.dtype.newbyteorder("=") != store:
                    raise ValueError("%s takes %s pictures, not %s" % (name, store.name, a.dtype))
                c, H, W = a.shape
                enc = StreamEncoder(c, H, W, settings, level, max_bits, dtype, batch, depth, ctx,
                                    _backend=_backend(c, H, W) if _backend else None)
            if a.shape != (enc.c, enc.H, enc.W):
                raise ValueError("picture %d has shape %s; picture 0 has %s" % (i, a.shape, (enc.c, enc.H, enc.W)))
            if a.dtype.newbyteorder("=") != store:
                raise ValueError("picture %d is %s; %s takes %s pictures" % (i, a.dtype, name, store.name))
            if buf is None:
                if enc.pending() == enc.depth:
                    yield from enc.next()
                buf, n = enc.input(), 0
            buf[n] = a
            n += 1
            if n == enc.batch:
                enc.submit(n)
                buf = None
        if buf is not None:
            enc.submit(n)
        while enc is not None and enc.pending():
            yield from enc.next()
    finally:
        if enc is not None:
            enc.close()


def encode_images(images, settings=None, level=None, max_bits=None, batch=32, depth=3, ctx=None, _backend=None):
    """An iterable of equally shaped float64 pictures (c, H, W) -> yields encode_image(picture, settings, level, max_bits)
    of each, in order, `batch` pictures per step with the transfers overlapped.  A picture of another shape: ValueError
    naming its index."""
    return _encode_stream(images, settings, level, max_bits, batch, depth, ctx, np.float64, "encode_images", _backend)


def encode_images_u8(images, settings=None, level=None, max_bits=None, batch=32, depth=3, ctx=None, _backend=None):
    """... uint8 pictures: encode_image_u8 of each"""
    return _encode_stream(images, settings, level, max_bits, batch, depth, ctx, np.uint8, "encode_images_u8", _backend)


def encode_images_u16(images, settings=None, level=None, max_bits=None, batch=32, depth=3, ctx=None, _backend=None):
    """... uint16 pictures: encode_image_u16 of each"""
    return _encode_stream(images, settings, level, max_bits, batch, depth, ctx, np.uint16, "encode_images_u16", _backend)


def encode_images_float(images, settings=None, level=None, max_bits=None, dtype=np.float32, batch=32, depth=3, ctx=None,
                        _backend=None):
    """... float32 / float16 pictures, or uint16 bit patterns with dtype="bfloat16": encode_image_float of each"""
    return _encode_stream(images, settings, level, max_bits, batch, depth, ctx, dtype, "encode_images_float", _backend)


def _decode_stream(results, settings, batch, depth, ctx, dtype, max_bytes, _backend):
    it = iter(results)
    dec = None
    try:
        def checked():
            nonlocal dec
            for i, r in enumerate(it):
                if dec is None:
                    dec = StreamDecoder(r.c, r.h, r.w, settings, r.level, dtype, batch, depth, ctx, max_bytes,
                                        _backend=_backend(r.c, r.h, r.w) if _backend else None)
                if (r.c, r.h, r.w, r.level) != (dec.c, dec.H, dec.W, dec.level):
                    raise ValueError("stream %d is of a picture (c, h, w, level) = %s; stream 0's is %s"
                                     % (i, (r.c, r.h, r.w, r.level), (dec.c, dec.H, dec.W, dec.level)))
                yield r
        groups = _batched(checked(), int(batch))
        first = next(groups, None)
        if first is None:
            return

        def chain():
            yield first
            yield from groups
        for pictures in dec.run(chain()):
            yield from pictures
    finally:
        if dec is not None:
            dec.close()


def decode_images(results, settings=None, batch=32, depth=3, ctx=None, max_bytes=None, _backend=None):
    """An iterable of EncodingResults of one geometry -> yields decode_image(result, settings) of each, in order (float64
    (c, H', W')), `batch` streams per step with the transfers overlapped.  A stream of another geometry: ValueError naming
    its index.  max_bytes: the longest stream to expect (None: the bound of the geometry; it sizes the page-locked staging)."""
    return _decode_stream(results, settings, batch, depth, ctx, np.float64, max_bytes, _backend)


def decode_images_u8(results, settings=None, batch=32, depth=3, ctx=None, max_bytes=None, _backend=None):
    """... decode_image_u8 of each: uint8 (c, H, W)"""
    return _decode_stream(results, settings, batch, depth, ctx, np.uint8, max_bytes, _backend)


def decode_images_u16(results, settings=None, batch=32, depth=3, ctx=None, max_bytes=None, _backend=None):
    """... decode_image_u16 of each: uint16 (c, H, W)"""
    return _decode_stream(results, settings, batch, depth, ctx, np.uint16, max_bytes, _backend)


def decode_images_float(results, settings=None, dtype=np.float32, batch=32, depth=3, ctx=None, max_bytes=None, _backend=None):
    """... decode_image_float(result, settings, dtype) of each: float32, float16, or uint16 bit patterns for bfloat16"""
    return _decode_stream(results, settings, batch, depth, ctx, dtype, max_bytes, _backend)
