"""irspack_amd — MI355X (gfx950) native implementation of irspack's compiled hot path.

The package mirrors the module paths the reference's Python imports
(``irspack.recommenders._ials_core``, ``._knn``,
``irspack.evaluation._core_evaluator``) on top of ``libirspack_amd.so`` (hand-written
HIP kernels behind the C ABI in ``include/irspack_amd.h``).  There is no CPU
fallback: compute entry points raise when no HIP device is visible.
"""

__version__ = "0.1.0"

_LAZY = ("rowwise_train_test_split", "df_to_sparse")  # of irspack_amd.utils, imported on first use


def __getattr__(name):
    if name in _LAZY:
        from . import utils

        return getattr(utils, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
