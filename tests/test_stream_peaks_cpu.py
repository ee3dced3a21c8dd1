"""tdoa_stream_peaks / tdoa_stream_est_device without a GPU: the library exports
both, their NULL checks come before any device call and name the cause, and
the ctypes prototypes exist."""
import ctypes as C
import os

import tdoa
from tdoa import _lib

NEW = ("tdoa_stream_peaks", "tdoa_stream_est_device")


def test_library_exports_the_symbols():
    L = tdoa.load()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "..", "include", "tdoa.h")).read()
    for name in NEW:
        assert f"int {name}(" in hdr, name


def test_prototypes():
    L = tdoa.load()
    P = C.c_void_p
    assert L.tdoa_stream_peaks.argtypes == [P, C.POINTER(_lib.PeaksParams), P, C.POINTER(_lib.PeaksOutputs), P]
    assert L.tdoa_stream_est_device.argtypes == [P, C.POINTER(P), C.POINTER(C.c_int)]
    from tdoa.stream import StreamPipeline
    for m in ("peaks", "peak_records", "peaks_all", "est_ptr"):
        assert callable(getattr(StreamPipeline, m))


def test_null_arguments_fail_without_a_device():
    L = tdoa.load()
    prm = _lib.PeaksParams(2, 8, 0.0)
    out = _lib.PeaksOutputs()
    assert L.tdoa_stream_peaks(None, C.byref(prm), None, C.byref(out), None) == -1
    msg = L.tdoa_last_error()
    assert msg and b"tdoa_stream_peaks" in msg and b"NULL" in msg
    assert L.tdoa_stream_peaks(None, None, None, None, None) == -1
    ptr, flt = C.c_void_p(), C.c_int(5)
    assert L.tdoa_stream_est_device(None, C.byref(ptr), C.byref(flt)) == -1
    msg = L.tdoa_last_error()
    assert msg and b"tdoa_stream_est_device" in msg and b"NULL" in msg
    assert ptr.value is None and flt.value == 5  # nothing written
