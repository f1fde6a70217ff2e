"""CPU side of the fused classifier tail (qnn_avgpool_dense_softmax_forward): the header declares it, the library exports it
without an ABI version step, and its pointer checks come before any device call (there is no GPU here)."""
import ctypes
import os
import re

from qnn_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qnn_avgpool_dense_softmax_forward"


def test_header_declares_and_library_exports_the_tail_entry():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qnn_abi.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert decl is not None, "include/qnn_abi.h does not declare " + NAME
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 14 and args[0].startswith("const qnn_weights_t*") and args[-1] == "void* stream", args
    assert hasattr(ctypes.CDLL(_abi.lib_path()), NAME)
    assert NAME in _abi.EXPORTS and len(_abi.EXPORTS) == 29
    lib = _abi.load()
    assert lib.qnn_version() == 4
    assert len(lib.qnn_avgpool_dense_softmax_forward.argtypes) == 14
    assert callable(_abi.avgpool_dense_softmax)


def test_null_pointers_are_rejected_before_any_device_call():
    lib = _abi.load()
    # stand-ins that are never dereferenced: the null check is the function's first statement
    fake = ctypes.create_string_buffer(256)
    p = ctypes.cast(fake, ctypes.c_void_p)
    epi = _abi.make_epilogue(None, None, _abi.FN_NONE, 0, 1, _abi.STORE_F32)
    for x, y in ((None, p), (p, None), (None, None)):
        rc = lib.qnn_avgpool_dense_softmax_forward(p, x, _abi.STORE_I4, 4, 1, 8, 8, 64, 8, ctypes.byref(epi), 1, None, y, None)
        assert rc == -1, rc                                   # QNN_EINVAL
        msg = lib.qnn_last_error().decode()
        assert NAME in msg and "null" in msg, msg
    rc = lib.qnn_avgpool_dense_softmax_forward(None, p, _abi.STORE_I4, 4, 1, 8, 8, 64, 8, ctypes.byref(epi), 1, None, p, None)
    assert rc == -1 and NAME in lib.qnn_last_error().decode()
