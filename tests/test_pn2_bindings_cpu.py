"""The PointNet++ bindings of _lib without a GPU: every `*_f32` wrapper names itself and the offending argument before it touches the
device, and every `*_workspace_bytes` function reaches its own C symbol with the right number of arguments (the library loads on the
host and answers sizing questions there)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import sub                           # noqa: E402
import pn2_bindings_util as U                      # noqa: E402


@pytest.mark.parametrize("name", U.WRAPPERS)
def test_cpu_tensors_are_refused_by_prefix_and_argument(name):
    L = sub("_lib")
    first = U.TENSOR_ARGS[name][0]
    with pytest.raises(L.AmpnetError, match=f"^{name}: {first} must be .*GPU"):
        U.call(L, name, U.valid_args(L, name, "cpu"))


@pytest.mark.parametrize("name", U.WRAPPERS)
def test_a_missing_required_tensor_is_named(name):
    """None where a tensor is required is an AmpnetError that names it, never an AttributeError or a ValueError."""
    L = sub("_lib")
    for missing in U.required(name):
        with pytest.raises(L.AmpnetError, match=f"^{name}: .*{missing}"):
            U.call(L, name, dict(U.valid_args(L, name, "cpu"), **{missing: None}))


SIZING = {"fp_backward": (U.D1, U.D2, U.B, U.N), "fp_train_forward": (U.D1, U.D2, U.B, U.N), "fp_train_backward": (U.D1, U.D2, U.B, U.N),
          "sa_backward": (U.D, U.B, U.S, U.NSAMPLE), "sa_train_forward": (U.D, U.B, U.S, U.NSAMPLE),
          "sa_train_backward": (U.D, U.B, U.S, U.NSAMPLE), "sa_all_forward": (U.D, U.B, U.N), "sa_all_backward": (U.D, U.B, U.N)}


@pytest.mark.parametrize("name", sorted(SIZING))
def test_workspace_bytes_reaches_its_symbol(name):
    L = sub("_lib")
    need = getattr(L, name + "_workspace_bytes")
    assert need(*SIZING[name], U.COUTS) > 0
    with pytest.raises(L.AmpnetError, match="multiple of 32"):
        need(*SIZING[name], [32, 48])
