"""Per-model matrix precision, the part that needs no GPU: the --precision flag of the six CLI files that take it (the three training CLI files and
the three infer_* CLI files; the reference-named test_* CLI files keep the reference's flags), _lib.resolve_precision, the
`precision` keyword of the model classes (stored, never in the state_dict) and the library's scoped override
(include/ampnet_hip.h: ampnet_precision_scope_begin / _end, ampnet_effective_matrix_precision) -- the library loads without a device,
so the scope stack is exercised here and not in tests/test_precision_gpu.py."""
import importlib.util
import os
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conftest import PKG, sub                      # noqa: E402

NAMES = ["fp32", "f32x3", "bf16", "bf16_train", "bf16_store"]
CLI_FILES = ["self-attention/train_pointnet-attention.py", "self-attention/infer_pointnet_att_segmen.py",
             "rnn/train_pointnetGRU.py", "rnn/infer_pointnet_gru_segmen.py",
             "baseline/train_segmentation.py", "baseline/infer_segmentation.py"]
# what each parser needs besides --precision (positional dataset folder, required flags)
CLI_ARGS = {"self-attention/train_pointnet-attention.py": ["data"], "baseline/train_segmentation.py": ["data"],
            "baseline/infer_segmentation.py": ["data", "--model_checkpoint", "ck.pth"]}


def _parser(rel):
    path = os.path.join(ROOT, PKG, "pointNet", rel)
    spec = importlib.util.spec_from_file_location("cli_" + os.path.basename(rel)[:-3].replace("-", "_"), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_parser()


@pytest.mark.parametrize("rel", CLI_FILES)
def test_cli_precision_flag(rel, capsys):
    parser = _parser(rel)
    base = CLI_ARGS.get(rel, [])
    assert parser.parse_args(base).precision is None
    for name in NAMES:
        assert parser.parse_args(base + ["--precision", name]).precision == name
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--precision", "fp8"])
    assert "fp8" in capsys.readouterr().err


@pytest.mark.parametrize("infer,ref", [("self-attention/infer_pointnet_att_segmen.py", "self-attention/test_pointnet_att_segmen.py"),
                                       ("rnn/infer_pointnet_gru_segmen.py", "rnn/test_pointnet_gru_segmen.py"),
                                       ("baseline/infer_segmentation.py", "baseline/test_segmentation.py")])
def test_infer_cli_keeps_the_flags_of_the_test_cli(infer, ref):
    """Every add_argument line of the reference-named CLI file is in the infer_* file, verbatim: same flags, types and defaults."""
    read = lambda rel: open(os.path.join(ROOT, PKG, "pointNet", rel)).read()                                        # noqa: E731
    want = [l.strip() for l in read(ref).splitlines() if ".add_argument(" in l]
    have = [l.strip() for l in read(infer).splitlines()]
    assert len(want) >= 6 and all(l in have for l in want)


def test_drivers_take_precision_last():
    """`precision=None` is the last keyword of the drivers that build their own models."""
    import inspect
    for mod, fn in (("pointNet.amp_train", "train_att"), ("pointNet.amp_infer", "test"), ("pointNet.gru_train", "train_gru"), ("pointNet.gru_train", "test"),
                    ("pointNet.baseline_seg", "train"), ("pointNet.baseline_seg", "test")):
        params = list(inspect.signature(getattr(sub(mod), fn)).parameters.values())
        assert params[-1].name == "precision" and params[-1].default is None, (mod, fn)
    for fn in ("fused_train_step", "Trainer"):
        assert inspect.signature(getattr(sub("trainer"), fn)).parameters["precision"].default is None


def test_resolve_precision_order(monkeypatch):
    L = sub("_lib")
    monkeypatch.delenv("AMPNET_PRECISION", raising=False)
    assert L.resolve_precision() is None and L.resolve_precision(None) is None
    assert L.resolve_precision("bf16") == "bf16"
    monkeypatch.setenv("AMPNET_PRECISION", "f32x3")
    assert L.resolve_precision() == "f32x3"
    assert L.resolve_precision("bf16_store") == "bf16_store"          # the explicit value wins over the environment
    monkeypatch.setenv("AMPNET_PRECISION", "")
    assert L.resolve_precision() is None
    with pytest.raises(ValueError) as e:
        L.resolve_precision("fp8")
    assert all(n in str(e.value) for n in NAMES)
    monkeypatch.setenv("AMPNET_PRECISION", "fp8")
    with pytest.raises(ValueError):
        L.resolve_precision()
    assert list(L.PRECISION_NAMES) == NAMES


def _model_classes():
    A, P, LP = sub("pointNet.model.pointnetAtt"), sub("pointNet.model.pointnet"), sub("pointNet.model.light_pointnet_256")
    return {
        "BasePointNet": lambda **k: A.BasePointNet(3, True, 256, "cpu", **k),
        "SegmentationWithAttention": lambda **k: A.SegmentationWithAttention(256, 8, 5, 64, 0.3, "cpu", **k),
        "SegmentationWithGRU": lambda **k: A.SegmentationWithGRU(5, 256, 64, "cpu", **k),
        "ClassificationWithAttention": lambda **k: A.ClassificationWithAttention(256, 8, 2, 0.3, 9, "cpu", **k),
        "pointnet.SegmentationPointNet": lambda **k: P.SegmentationPointNet(5, 3, "cpu", **k),
        "pointnet.ClassificationPointNet": lambda **k: P.ClassificationPointNet(5, 0.3, 3, "", "cpu", **k),
        "light.SegmentationPointNet": lambda **k: LP.SegmentationPointNet(5, 2, "cpu", **k),
        "light.ClassificationPointNet": lambda **k: LP.ClassificationPointNet(5, 0.3, 2, "", "cpu", **k),
    }


@pytest.mark.parametrize("name", ["BasePointNet", "SegmentationWithAttention", "SegmentationWithGRU", "ClassificationWithAttention",
                                  "pointnet.SegmentationPointNet", "pointnet.ClassificationPointNet",
                                  "light.SegmentationPointNet", "light.ClassificationPointNet"])
def test_model_precision_kwarg(name):
    make = _model_classes()[name]
    plain, with_kw = make(), make(precision="bf16_store")
    assert plain.precision is None and with_kw.precision == "bf16_store"
    assert list(plain.state_dict().keys()) == list(with_kw.state_dict().keys())
    assert [k for k, _ in plain.named_parameters()] == [k for k, _ in with_kw.named_parameters()]
    assert [k for k, _ in plain.named_buffers()] == [k for k, _ in with_kw.named_buffers()]
    assert with_kw.set_precision("f32x3") is with_kw and with_kw.precision == "f32x3"
    assert list(plain.state_dict().keys()) == list(with_kw.state_dict().keys())
    with_kw.set_precision(None)
    assert with_kw.precision is None
    with pytest.raises(ValueError):
        make(precision="fp8")
    with pytest.raises(ValueError):
        plain.set_precision("fp8")


def test_precision_is_keyword_only():
    """It comes after the reference's arguments and cannot be reached positionally, so positional use is unchanged."""
    import inspect
    A, P, LP = sub("pointNet.model.pointnetAtt"), sub("pointNet.model.pointnet"), sub("pointNet.model.light_pointnet_256")
    for cls in (A.BasePointNet, A.SegmentationWithAttention, A.SegmentationWithGRU, A.ClassificationWithAttention,
                P.SegmentationPointNet, P.ClassificationPointNet, LP.SegmentationPointNet, LP.ClassificationPointNet):
        par = inspect.signature(cls.__init__).parameters
        assert par["precision"].kind is inspect.Parameter.KEYWORD_ONLY and par["precision"].default is None, cls
        assert list(par)[-1] == "precision", cls


def test_trainer_refuses_a_mixed_tape_without_a_device():
    """'bf16_store' on one module only: ValueError from the check that runs before any launch (no GPU is touched to get there)."""
    A, T = sub("pointNet.model.pointnetAtt"), sub("trainer")
    enc = A.BasePointNet(3, True, 256, "cpu", precision="bf16_store")
    att = A.SegmentationWithAttention(256, 8, 5, 64, 0.3, "cpu", precision="fp32")
    with pytest.raises(ValueError, match="bf16_store"):
        T.step_precision(enc, att)
    att.set_precision("bf16_store")
    assert T.step_precision(enc, att) == ("bf16_store", "bf16_store")
    att.set_precision(None)                                          # None follows the default: nothing to compare before the launch
    assert T.step_precision(enc, att) == ("bf16_store", None)
    att.set_precision("f32x3"); enc.set_precision("bf16")           # both keep an fp32 tape
    assert T.step_precision(enc, att) == ("bf16", "f32x3")


# ---- the library's scope stack -----------------------------------------------------------------------------------------------------
@pytest.fixture
def lib():
    L = sub("_lib")
    lib = L.lib()
    assert lib.ampnet_get_matrix_precision() == 0 and lib.ampnet_effective_matrix_precision() == 0
    yield lib
    while lib.ampnet_precision_scope_end() == 0:                     # a failed test leaves no scope behind
        pass
    assert lib.ampnet_effective_matrix_precision() == lib.ampnet_get_matrix_precision() == 0


def test_scope_round_trip(lib):
    L = sub("_lib")
    for name in NAMES:
        code = L.PRECISIONS[name]
        assert lib.ampnet_precision_scope_begin(code) == 0
        assert lib.ampnet_effective_matrix_precision() == code
        assert lib.ampnet_get_matrix_precision() == 0                # the process-wide default is not the scope's business
        assert lib.ampnet_precision_scope_end() == 0
        assert lib.ampnet_effective_matrix_precision() == 0
    # nested scopes: the innermost wins, each end uncovers the one below
    assert lib.ampnet_precision_scope_begin(4) == 0 and lib.ampnet_precision_scope_begin(3) == 0
    assert lib.ampnet_effective_matrix_precision() == 3
    assert lib.ampnet_precision_scope_end() == 0
    assert lib.ampnet_effective_matrix_precision() == 4
    assert lib.ampnet_precision_scope_end() == 0
    # the default shows through an empty stack, and a scope hides a default changed underneath it
    try:
        assert lib.ampnet_set_matrix_precision(1) == 0
        assert lib.ampnet_effective_matrix_precision() == 1
        assert lib.ampnet_precision_scope_begin(0) == 0
        assert lib.ampnet_set_matrix_precision(2) == 0
        assert lib.ampnet_effective_matrix_precision() == 0 and lib.ampnet_get_matrix_precision() == 2
        assert lib.ampnet_precision_scope_end() == 0
        assert lib.ampnet_effective_matrix_precision() == 2
    finally:
        lib.ampnet_set_matrix_precision(0)


def test_scope_errors(lib):
    assert lib.ampnet_precision_scope_end() == -1                    # AMPNET_E_ARG: nothing pushed
    assert b"no scope" in lib.ampnet_last_error()
    for bad in (-1, 5, 99):
        assert lib.ampnet_precision_scope_begin(bad) == -1
        assert lib.ampnet_effective_matrix_precision() == 0
    assert lib.ampnet_precision_scope_end() == -1                    # the refused begins pushed nothing
    for depth in range(8):
        assert lib.ampnet_precision_scope_begin(1 + depth % 4) == 0, depth
    assert lib.ampnet_precision_scope_begin(1) == -1                 # the ninth: an error, not a crash, and nothing changes
    assert b"nested" in lib.ampnet_last_error()
    assert lib.ampnet_effective_matrix_precision() == 1 + 7 % 4
    for depth in range(8):
        assert lib.ampnet_precision_scope_end() == 0
    assert lib.ampnet_precision_scope_end() == -1
    assert lib.ampnet_effective_matrix_precision() == 0


def test_scope_is_per_thread(lib):
    seen = {}

    def other():
        seen["before"] = lib.ampnet_effective_matrix_precision()
        seen["end"] = lib.ampnet_precision_scope_end()               # this thread has pushed nothing
        seen["begin"] = lib.ampnet_precision_scope_begin(3)
        seen["inside"] = lib.ampnet_effective_matrix_precision()
        gate.set()
        done.wait(10)
        seen["closed"] = lib.ampnet_precision_scope_end()

    gate, done = threading.Event(), threading.Event()
    assert lib.ampnet_precision_scope_begin(4) == 0
    t = threading.Thread(target=other)
    t.start()
    assert gate.wait(10)
    mine = lib.ampnet_effective_matrix_precision()                   # the other thread's scope (3) is open right now
    done.set()
    t.join(10)
    assert lib.ampnet_precision_scope_end() == 0
    assert mine == 4
    assert seen == {"before": 0, "end": -1, "begin": 0, "inside": 3, "closed": 0}


def test_precision_scope_context_manager(lib):
    L = sub("_lib")
    with L.precision_scope(None):                                    # no-op
        assert L.effective_matrix_precision() == "fp32"
    with L.precision_scope("f32x3"):
        assert L.effective_matrix_precision() == "f32x3" and L.get_matrix_precision() == "fp32"
        with L.precision_scope("bf16_store"):
            assert L.effective_matrix_precision() == "bf16_store"
        assert L.effective_matrix_precision() == "f32x3"
    assert L.effective_matrix_precision() == "fp32"
    with pytest.raises(RuntimeError, match="boom"):
        with L.precision_scope("bf16"):
            raise RuntimeError("boom")
    assert L.effective_matrix_precision() == "fp32"                  # closed although the body raised
    with pytest.raises(ValueError):
        with L.precision_scope("fp8"):
            pass
    assert lib.ampnet_precision_scope_end() == -1                    # and the refused name opened nothing


def test_header_and_binding_agree_on_the_abi_version():
    import re
    L = sub("_lib")
    text = open(os.path.join(ROOT, "include", "ampnet_hip.h")).read()
    assert int(re.search(r"#define AMPNET_ABI_VERSION (\d+)", text).group(1)) == L.ABI_VERSION == L.lib().ampnet_abi_version()
    for sym in ("ampnet_precision_scope_begin", "ampnet_precision_scope_end", "ampnet_effective_matrix_precision"):
        assert re.search(r"\bint " + sym + r"\(", text) and hasattr(L.lib(), sym)
