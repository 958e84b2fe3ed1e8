"""The C ABI of the native feature-aware epoch without a GPU: the three entry points are declared
in the header, exported by the library, listed and typed in ``_lib``, and reject a null trainer
with an error status and message."""
import ctypes as C
import os
import re

from irspack_amd import _lib

NEW = ("irs_ials_feature_step", "irs_ials_get_feature_weight", "irs_ials_set_feature_weight")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "irspack_amd.h")


def test_declared_exported_and_typed():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(irs_\w+)\s*\(", f.read()))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.ARGTYPES[name] and fn.restype is C.c_int32
    assert len(_lib.ARGTYPES["irs_ials_set_feature_weight"]) == 5


def test_null_trainer_is_an_error():
    lib = _lib.lib()
    sc = _lib.SolverConfigStruct(1, 0, 3, 64, 1)
    assert lib.irs_ials_feature_step(None, C.byref(sc)) == 1
    assert lib.irs_last_error() == b"null trainer."
    assert lib.irs_ials_get_feature_weight(None, 0, None) == 1
    assert lib.irs_ials_set_feature_weight(None, 0, None, 0, 0) == 1
