"""CPU tests: the C-ABI library loads and exports every symbol include/spiht_hip.h declares; the Python
boundary mirrors the reference's names and argument checking.  No compute calls (no GPU here)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "spiht_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(spiht_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from spiht_amd import _lib
    L = _lib.lib()
    declared = _declared_symbols()
    assert len(declared) >= 25
    for s in declared:
        assert hasattr(L, s), "libspiht_hip.so does not export %s" % s
    assert sorted(_lib.SYMBOLS) == declared
    assert L.spiht_abi_version() == 2
    # the shipped library is not a diagnostic build (-DSPIHT_DIAG -DDEC_PROF: timers inside the list decoder's loops,
    # tools/prof_decode.py): its entry points are not there
    for s in ("spiht_debug_words", "spiht_debug_words_ext"):
        assert not hasattr(L, s), "libspiht_hip.so is a diagnostic build (%s)" % s


def _header_text():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "spiht_hip.h")).read(), flags=re.S)


def _ctypes_class(t):
    """a ctypes argument or result type in the words of the probe below"""
    import ctypes as C
    if t is None:
        return "void"
    if t is C.c_char_p:
        return "str"
    if t is C.c_void_p:
        return "ptr"
    if t in (C.c_float, C.c_double, C.c_longdouble):
        return "f%d" % C.sizeof(t)
    return "%s%d" % ("i" if t(-1).value < 0 else "u", C.sizeof(t))


PROBE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "spiht_hip.h"
template <class T> void cls() {
    if constexpr (std::is_void<T>::value) printf(" void");
    else if constexpr (std::is_pointer<T>::value)
        printf(std::is_same<typename std::remove_cv<typename std::remove_pointer<T>::type>::type, char>::value ? " str" : " ptr");
    else if constexpr (std::is_floating_point<T>::value) printf(" f%zu", sizeof(T));
    else if constexpr (std::is_integral<T>::value) printf(" %c%zu", std::is_signed<T>::value ? 'i' : 'u', sizeof(T));
    else printf(" other");
}
template <class R, class... A> void sig(const char *name, R (*)(A...)) {
    printf("%s", name);
    cls<R>();
    (cls<A>(), ...);
    printf("\n");
}
#define FIELD(S, F) printf(" %s:%zu:%zu", #F, offsetof(S, F), sizeof(((S *)0)->F))
int main() {
@BODY@
    return 0;
}
"""


def test_binding_is_the_compilers_view_of_the_header(tmp_path):
    """Every entry point's argtypes and restype, and the three Structure classes, against what a C++ compiler makes of the header:
    a host program deduces each prototype's result and parameters (pointer to char; other pointer; floating point or signed /
    unsigned integer of a size; void) and prints each struct's size and its fields' offsets and sizes.  It takes the address of
    every entry point, so it links against the library; it calls none."""
    import ctypes as C
    import shutil
    import subprocess
    from spiht_amd import _lib
    L = _lib.lib()
    declared = _declared_symbols()
    body = ['    sig("%s", &%s);' % (s, s) for s in declared]
    for name, cls in _lib.STRUCTS.items():
        body.append('    printf("struct %s %%zu", sizeof(%s));' % (name, name))
        body += ["    FIELD(%s, %s);" % (name, f) for f, _ in cls._fields_]
        body.append('    printf("\\n");')
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE.replace("@BODY@", "\n".join(body)))
    cxx = shutil.which("c++") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe"),
                           os.path.abspath(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
    lines = subprocess.check_output([str(tmp_path / "probe")], text=True).splitlines()
    seen = {ln.split()[0]: ln.split()[1:] for ln in lines if not ln.startswith("struct ")}
    assert sorted(seen) == declared and len(declared) >= 192
    for s in declared:
        fn = getattr(L, s)
        assert [_ctypes_class(fn.restype)] + [_ctypes_class(t) for t in fn.argtypes] == seen[s], s
    structs = {ln.split()[1]: ln.split()[2:] for ln in lines if ln.startswith("struct ")}
    assert sorted(structs) == sorted(_lib.STRUCTS)
    for name, cls in _lib.STRUCTS.items():
        here = [str(C.sizeof(cls))] + ["%s:%d:%d" % (f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
        assert here == structs[name], name


def test_no_entry_point_is_left_unbound():
    """a function without argtypes takes every Python integer as a 32-bit int: every declared name has a list, empty exactly for
    the (void) functions, and the result type its prototype says"""
    import ctypes as C
    from spiht_amd import _lib
    L = _lib.lib()
    text = _header_text()
    for s in _lib.SYMBOLS:
        ret, params = re.search(r"(\bconst\s+char\s*\*|\bvoid\b|\bint\b)\s*%s\s*\(([^)]*)\)" % s, text).groups()
        fn = getattr(L, s)
        assert isinstance(fn.argtypes, list), s
        assert (len(fn.argtypes) == 0) == (params.strip() == "void"), s
        assert len(fn.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), s
        assert fn.restype is {"void": None, "int": C.c_int}.get(ret, C.c_char_p), s


def test_structures_match_the_header():
    from spiht_amd import _header, _lib
    text = open(_lib.HEADER_PATH).read()
    structs = _header.parse(text)[1]
    assert sorted(structs) == sorted(_lib.STRUCTS) and len(structs) == 3
    for name, cls in _lib.STRUCTS.items():
        assert cls._fields_ == structs[name], name
        body = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}" % name, _header_text()).group(1)
        assert [f for f, _ in cls._fields_] == re.findall(r"(\w+)\s*[,;]", body), name
    _lib.check_structs(structs)
    # two fields of one struct swapped, in a copy of the text: the check lib() makes refuses the library
    swapped = text.replace("int64_t n; ", "@").replace("uint64_t nbytes;", "int64_t n;").replace("@", "uint64_t nbytes; ")
    assert swapped != text and len(swapped) == len(text)
    with pytest.raises(ImportError, match="HStreamResult"):
        _lib.check_structs(_header.parse(swapped)[1])


def test_constants_are_the_headers_enumerators():
    from spiht_amd import _lib
    L = _lib.lib()
    found = re.findall(r"\b(SPIHT_(?:OK|ERR_\w+|MODE_\w+|HS_\w+))\s*=\s*(\d+)", _header_text())
    assert len(found) >= 31 and len(set(n for n, _ in found)) == len(found)
    for name, value in found:
        assert _lib.ENUMS[name] == int(value), name
        if name == "SPIHT_OK" or name.startswith("SPIHT_ERR_"):
            assert getattr(_lib, name[len("SPIHT_"):]) == int(value), name
    assert len(_lib.ENUMS) == len(found)
    modes = {n[len("SPIHT_MODE_"):].lower(): int(v) for n, v in found if n.startswith("SPIHT_MODE_")}
    assert _lib.MODES == modes and len(modes) == 9
    for name in modes:
        assert L.spiht_mode_id(name.encode()) == _lib.MODES[name], name


def test_parser_refuses_a_type_it_does_not_know():
    from spiht_amd import _header
    ok = "int spiht_fine(int64_t n, const char *name, spiht_ctx **out);\n"
    assert list(_header.parse(ok)[0]) == ["spiht_fine"]
    for bad in ("int spiht_odd(int64_t n, long double q);", "int spiht_odd(int64_t n, size_t q);", "int spiht_odd(float);",
                "long double spiht_odd(int n);", "int spiht_odd(unsigned n);"):
        with pytest.raises(ValueError, match="spiht_odd"):
            _header.parse(ok + bad)


def test_package_surface_matches_reference_init():
    import spiht_amd
    # /root/reference/spiht/__init__.py:1-2
    for name in ["encode_image", "decode_image", "EncodingResult", "SpihtSettings", "ENCODER_DECODER_VERSION", "encode",
                 "decode"]:
        assert hasattr(spiht_amd, name)
    s = spiht_amd.SpihtSettings()
    assert (s.wavelet, s.quantization_scale, s.mode, s.color_model, s.per_channel_quant_scales) == \
        ("bior2.2", 50.0, "reflect", None, None)
    # positional order is API (demonstrate.py:23-29)
    s = spiht_amd.SpihtSettings("bior4.4", 1.0, "symmetric", "IPT", [100., 20., 20.])
    assert s.mode == "symmetric" and s.per_channel_quant_scales == [100., 20., 20.]
    assert spiht_amd.ENCODER_DECODER_VERSION == "0.0.2"
    r = spiht_amd.EncodingResult(b"ab", 4, 5, 3, 7, None)
    d = r.to_dict()
    assert d["encoding_result_h"] == 4 and d["encoding_result__encoding_version"] == "0.0.2"
    assert spiht_amd.EncodingResult.from_dict(d) == r


def test_geometry_and_bound_without_gpu():
    """host-only entry points of the C ABI (no device needed)"""
    import ctypes as C
    from spiht_amd import _lib
    from spiht_amd.spiht_wrapper import SpihtSettings, get_slices_and_h_w
    L = _lib.lib()
    # SURVEY.md App. A
    for (H, W, wv, lv, ll, enc) in [(512, 512, "bior2.2", 5, (20, 20), (533, 533)),
                                    (1080, 1920, "bior2.2", 7, (13, 19), (1111, 1949)),
                                    (1024, 1024, "bior2.2", None, (12, 12), (1053, 1053)),
                                    (4096, 4096, "bior6.8", 9, (24, 24), (4241, 4241))]:
        slices, eh, ew = get_slices_and_h_w(H, W, SpihtSettings(wavelet=wv), lv)
        assert (slices[0][1].stop, slices[0][2].stop) == ll and (eh, ew) == enc
    b = C.c_uint64()
    assert L.spiht_encode_bound(3, 1111, 1949, 13, 19, 6485, 1036800, C.byref(b)) == 0
    assert b.value == 129600
    assert L.spiht_encode_bound(3, 1111, 1949, 13, 19, 6485, 0, C.byref(b)) == 0
    assert b.value > 3 * 1111 * 1949 // 8
    assert L.spiht_encode_bound(1, 8, 8, 1, 2, 5, 0, C.byref(b)) == _lib.ERR_LL
    assert L.spiht_encode_bound(1, 6, 8, 4, 2, 5, 0, C.byref(b)) == _lib.ERR_SHAPE
    assert L.spiht_wavelet_id(b"bior2.2") >= 0 and L.spiht_wavelet_id(b"nope") < 0
    assert L.spiht_mode_id(b"reflect") == 0 and L.spiht_mode_id(b"smooth") == 5 and L.spiht_mode_id(b"periodization") == 8 and L.spiht_mode_id(b"nope") < 0


def test_geometry_matches_golden_pywt_shapes():
    from spiht_amd.spiht_wrapper import SpihtSettings, get_slices_and_h_w
    w = np.load(os.path.join(ROOT, "tests", "golden", "wrapper_pywt.npz"))
    names = ["bior2.2", "bior4.4", "bior6.8", "haar"]
    for row in w["geometry"]:
        H, W, wi, lv, llh, llw, eh, ew, nlev = [int(v) for v in row]
        slices, gh, gw = get_slices_and_h_w(H, W, SpihtSettings(wavelet=names[wi]), None if lv < 0 else lv)
        assert (slices[0][1].stop, slices[0][2].stop, gh, gw, len(slices) - 1) == (llh, llw, eh, ew, nlev)


def test_argument_checking_mirrors_pyo3():
    import spiht_amd
    from spiht_amd.spiht import PanicException
    with pytest.raises(TypeError):
        spiht_amd.encode([[1, 2], [3, 4]], 2, 2, 10)
    with pytest.raises(TypeError):
        spiht_amd.encode(np.zeros((1, 8, 8), np.int64), 2, 2, 10)
    with pytest.raises(TypeError):
        spiht_amd.encode(np.zeros((8, 8), np.int32), 2, 2, 10)
    with pytest.raises(OverflowError):
        spiht_amd.encode(np.zeros((1, 8, 8), np.int32), 2, 2, -1)
    with pytest.raises(TypeError):
        spiht_amd.decode("abc", 3, 1, 8, 8, 2, 2)
    with pytest.raises(PanicException):
        spiht_amd.decode(b"\x00", 3, 1, 8, 8, 1, 2)
    with pytest.raises(ValueError):
        spiht_amd.encode_image(np.zeros((8, 8)))
    with pytest.raises(ValueError):
        spiht_amd.decode_image(spiht_amd.EncodingResult(b"", 8, 8, 1, 0, None, "0.0.1"), spiht_amd.SpihtSettings())


def test_no_silent_cpu_fallback():
    """Without a GPU the product path must raise, not compute."""
    import spiht_amd
    from spiht_amd import _lib
    try:
        _lib.Context(0).close()
        pytest.skip("a GPU is present")
    except _lib.SpihtHipError:
        pass
    with pytest.raises(_lib.SpihtHipError):
        spiht_amd.encode(np.ones((1, 8, 8), np.int32), 2, 2, 100)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "spiht_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "liboracle" not in txt, f
