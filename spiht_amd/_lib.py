"""ctypes binding of libspiht_hip.so.  include/spiht_hip.h is the binding: the first lib() reads it (_header.py) and gives every
entry point it declares its argtypes and restype, so a call is added by declaring it there and nowhere else.  SYMBOLS, the
status codes OK / ERR_*, MODES and ENUMS below are that parse's results, there once lib() has run -- importing the package
runs it.  Only the three Structure classes repeat the header, for their field names; lib() checks them against it.

The HIP library is the only compute path of this package: if it is missing or cannot be loaded the
import fails loudly -- there is no CPU fallback (the CPU restatement under oracle/ is test
infrastructure and is never imported from here).
"""
import ctypes as C
import os
import threading

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPIHT_HIP_LIB") or os.path.join(_HERE, "libspiht_hip.so")  # override: diagnostic builds

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "spiht_hip.h")  # the tree is used in place

SYMBOLS = []  # every entry point the header declares, in its order
ENUMS = {}    # every enumerator of the header by its name there: SPIHT_OK, SPIHT_ERR_*, SPIHT_MODE_*, SPIHT_HS_*
MODES = {}    # the pywt name of a signal extension mode -> SPIHT_MODE_*
# OK, ERR_LL ... ERR_IDLE: SPIHT_OK and every SPIHT_ERR_* under these names, module attributes set by lib()


class SpihtHipError(RuntimeError):
    """A HIP runtime failure or an internal guard of libspiht_hip."""


class PanicException(BaseException):
    """Counterpart of pyo3_runtime.PanicException, which the reference raises when the Rust core panics
    (assert!(ll_h > 1), encoder_decoder.rs:160-161; out-of-bounds index; unwrap on an empty array).
    Like PyO3's, it derives from BaseException."""


_lib = None
_lib_lock = threading.Lock()


class HStreamResult(C.Structure):
    """spiht_hstream_result"""
    _fields_ = [("n", C.c_int64), ("nbytes", C.c_uint64), ("bytes", C.c_void_p), ("lens", C.c_void_p), ("max_n", C.c_void_p),
                ("pictures", C.c_void_p), ("step", C.c_uint64)]


class TileSetPic(C.Structure):
    """spiht_tileset_pic: one picture of spiht_tile_cut_set"""
    _fields_ = [("d_img", C.c_void_p), ("sc", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64), ("H", C.c_int64), ("W", C.c_int64)]


class TileSetItem(C.Structure):
    """spiht_tileset_item: one window of spiht_tile_paste_set"""
    _fields_ = [("d_out", C.c_void_p), ("sc", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64), ("H", C.c_int64), ("W", C.c_int64),
                ("i0", C.c_int64), ("i1", C.c_int64), ("j0", C.c_int64), ("j1", C.c_int64),
                ("y0", C.c_int64), ("x0", C.c_int64), ("wh", C.c_int64), ("ww", C.c_int64)]


STRUCTS = {"spiht_hstream_result": HStreamResult, "spiht_tileset_pic": TileSetPic, "spiht_tileset_item": TileSetItem}


def check_structs(structs):
    """the Structure classes above against the header's structs (_header.parse): names, order and types of the fields"""
    for name, cls in STRUCTS.items():
        if cls._fields_ != structs.get(name):
            raise ImportError("spiht_amd._lib.%s is not the header's %s: %s there, %s here"
                              % (cls.__name__, name, structs.get(name), cls._fields_))


def lib():
    """Load libspiht_hip.so and bind it by the header (once).  Raises ImportError if either is missing or they disagree."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libspiht_hip.so is missing (%s): build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C spiht_amd/csrc`; spiht_amd has no CPU fallback" % LIB_PATH)
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:
            raise ImportError("cannot load %s: %s" % (LIB_PATH, e))
        try:
            with open(HEADER_PATH) as f:
                text = f.read()
        except OSError as e:
            raise ImportError("include/spiht_hip.h is missing (%s): the binding of libspiht_hip.so is read from it, and "
                              "spiht_amd is used in place, from its source tree" % e)
        functions, structs, enums = _header.parse(text)
        check_structs(structs)
        for name, (restype, argtypes) in functions.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise ImportError("%s does not export %s, which include/spiht_hip.h declares: rebuild it" % (LIB_PATH, name))
            fn.restype, fn.argtypes = restype, argtypes
        SYMBOLS[:] = functions
        ENUMS.update(enums)
        MODES.update((k[len("SPIHT_MODE_"):].lower(), v) for k, v in enums.items() if k.startswith("SPIHT_MODE_"))
        globals().update((k[len("SPIHT_"):], v) for k, v in enums.items() if k == "SPIHT_OK" or k.startswith("SPIHT_ERR_"))
        _lib = L
        return _lib


def check(status):
    """Map a C status to the exception the reference would raise."""
    if status == OK:
        return
    L = lib()
    msg = L.spiht_strerror(status).decode()
    if status in (ERR_LL, ERR_EMPTY, ERR_SHAPE):
        raise PanicException(msg)
    if status == ERR_HIP:
        raise SpihtHipError("%s: %s" % (msg, L.spiht_last_hip_error().decode()))
    if status in (ERR_INTERNAL, ERR_NOMEM):
        raise SpihtHipError("%s (%s)" % (msg, L.spiht_last_hip_error().decode()))
    if status == ERR_TOO_LARGE:
        raise OverflowError(msg)
    raise ValueError(msg)


class Context:
    """One spiht_ctx (device id, stream, scratch).  Created lazily, one per device."""

    def __init__(self, device=0, priority=0):
        self._lib = lib()
        h = C.c_void_p()
        check(self._lib.spiht_ctx_create_priority(int(device), int(priority), C.byref(h)))
        self.handle = h
        self.device = int(device)

    @classmethod
    def borrowed(cls, handle, device=0):
        """a view of a context someone else owns (e.g. a pipeline's): never destroyed from here"""
        self = cls.__new__(cls)
        self._lib = lib()
        self.handle = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self.device = int(device)
        self._borrowed = True
        return self

    def close(self):
        if getattr(self, "handle", None):
            if not getattr(self, "_borrowed", False):
                self._lib.spiht_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lock(self):
        """hold the context's (recursive) mutex across several calls of this thread: other threads' calls on the context
        wait until unlock() -- for settings that are state of the context (color_models.fused)"""
        check(self._lib.spiht_ctx_lock(self.handle))

    def unlock(self):
        check(self._lib.spiht_ctx_unlock(self.handle))

    def set_option(self, name, value):
        """a switch of the library (spiht_ctx_set_option): "l1_flags", "pads_persist", "wide_encode", "wide_groups",
        "wide_solo", "idwt_groups", "meta_chunk"; results do not depend on them"""
        check(self._lib.spiht_ctx_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int64()
        check(self._lib.spiht_ctx_get_option(self.handle, name.encode(), C.byref(v)))
        return int(v.value)

    def wide_stats(self):
        """(images, images that fell back to the single-workgroup encoder) of the last several-CUs-per-image encode call"""
        g, u = C.c_uint32(), C.c_uint32()
        check(self._lib.spiht_ctx_wide_stats(self.handle, C.byref(g), C.byref(u)))
        return int(g.value), int(u.value)

    def set_decoder_waves(self, waves):
        """wavefronts per decoder workgroup on this context: 12 (default, fastest alone) or 8 (lighter beside HBM-bound
        kernels of other contexts)"""
        check(self._lib.spiht_ctx_set_decoder_waves(self.handle, int(waves)))

    def wait_on(self, other):
        """device-side ordering: work queued on self after this call waits for work queued on `other` before it"""
        check(self._lib.spiht_ctx_wait_on(self.handle, other.handle))

    def synchronize(self):
        check(self._lib.spiht_ctx_synchronize(self.handle))

    def stream_ptr(self):
        """the context's hipStream_t as an integer (e.g. for torch.cuda.ExternalStream)"""
        p = C.c_void_p()
        check(self._lib.spiht_ctx_stream(self.handle, C.byref(p)))
        return p.value or 0

    def record(self, event=None):
        """mark the point this context's queue has reached; returns the Event (a new one unless given)"""
        if event is None:
            event = Event(self)
        check(self._lib.spiht_event_record(event.handle, self.handle))
        return event

    def wait_event(self, event):
        """work queued on this context from now on starts only after the recorded point"""
        check(self._lib.spiht_ctx_wait_event(self.handle, event.handle))

    # stage timing (HIP events on the context's stream)
    def set_timing(self, on):
        check(self._lib.spiht_ctx_set_timing(self.handle, 1 if on else 0))

    def reset_timing(self):
        check(self._lib.spiht_ctx_reset_timing(self.handle))

    def timing(self):
        out = {}
        for s in range(self._lib.spiht_ctx_num_stages()):
            ms, n = C.c_double(), C.c_uint64()
            check(self._lib.spiht_ctx_get_timing(self.handle, s, C.byref(ms), C.byref(n)))
            out[self._lib.spiht_ctx_stage_name(s).decode()] = (ms.value, n.value)
        return out

    # device memory helpers
    def alloc(self, nbytes):
        p = C.c_void_p()
        check(self._lib.spiht_dev_alloc(self.handle, int(nbytes), C.byref(p)))
        return p.value

    def free(self, ptr):
        check(self._lib.spiht_dev_free(self.handle, C.c_void_p(ptr)))

    def upload(self, dptr, arr):
        check(self._lib.spiht_dev_upload(self.handle, C.c_void_p(dptr), C.c_void_p(arr.ctypes.data), arr.nbytes))

    def download(self, arr, dptr):
        check(self._lib.spiht_dev_download(self.handle, C.c_void_p(arr.ctypes.data), C.c_void_p(dptr), arr.nbytes))

    def memset(self, dptr, value, nbytes):
        check(self._lib.spiht_dev_memset(self.handle, C.c_void_p(dptr), int(value), int(nbytes)))


class Event:
    """spiht_event: a point in one context's queue that other contexts can wait for (device-side)."""

    def __init__(self, ctx):
        self._lib = lib()
        h = C.c_void_p()
        check(self._lib.spiht_event_create(ctx.handle, C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._lib.spiht_event_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


_ctxs = {}
_ctx_lock = threading.Lock()


def _host_free(ptr):
    try:
        if _lib is not None:
            _lib.spiht_host_free(C.c_void_p(ptr))
    except Exception:  # interpreter shutdown
        pass


def result_array(shape, dtype):
    """An uninitialised array for a call to fill and RETURN (the reference's decode calls return new arrays,
    spiht_wrapper.py:192-216, lib.rs:35-42): backed by page-locked memory from the library's pool (spiht_host_alloc), so
    the device -> host copy is one DMA at the link's speed; the buffer goes back to the pool when the array -- and every
    view of it -- is gone.  Small arrays, or when no such memory is to be had: an ordinary numpy array."""
    import weakref
    import numpy as np
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if nbytes < (1 << 20):
        return np.empty(shape, dtype)
    p = C.c_void_p()
    if lib().spiht_host_alloc(nbytes, C.byref(p)) != OK or not p.value:
        return np.empty(shape, dtype)
    buf = (C.c_char * nbytes).from_address(p.value)
    weakref.finalize(buf, _host_free, p.value)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def default_context(device=None):
    if device is None:
        device = int(os.environ.get("SPIHT_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _ctx_lock:
        c = _ctxs.get(device)
        if c is None or c.handle is None:
            c = Context(device)
            if os.environ.get("SPIHT_DECODER_WAVES"):  # test runs of the whole suite on the 8-wavefront decoder
                c.set_decoder_waves(int(os.environ["SPIHT_DECODER_WAVES"]))
            _ctxs[device] = c
        return c
