"""CPU: the HistoryArch entries (csrc/history_arch.hip) are declared, exported and bound, say what they support, and
return argument errors before anything is launched."""
import _paths  # noqa: F401
from fbgemm_gpu import _lib
from test_abi import declared_symbols

NAMES = ("tbe_history_supported", "tbe_history_forward_f32", "tbe_history_backward_workspace_bytes", "tbe_history_backward_f32")


def test_the_entries_are_declared_exported_and_bound():
    lib = _lib.load()
    for n in NAMES:
        assert n in declared_symbols() and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert lib.tbe_abi_version() == 3


def test_supported_shapes_and_workspace():
    lib = _lib.load()
    for L, E in ((100, 256), (200, 128), (137, 128), (3, 4), (32, 1024), (128, 256), (16, 2048)):
        assert lib.tbe_history_supported(L, E) == 1, (L, E)
    for L, E in ((129, 256), (8, 6), (8, 2), (0, 16), (1, 4096), (1 << 40, 1 << 40)):
        assert lib.tbe_history_supported(L, E) == 0, (L, E)
    assert lib.tbe_history_backward_workspace_bytes(128, 100, 256, 0) == 0  # frozen parameters: no workspace
    assert lib.tbe_history_backward_workspace_bytes(128, 100, 256, 7) == 128 * 3 * 25600 * 4  # one sample per workgroup
    assert lib.tbe_history_backward_workspace_bytes(1024, 100, 256, 2) == 256 * 3 * 25600 * 4  # four of them


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    fwd = lambda B, N, L, E, p, eps: lib.tbe_history_forward_f32(  # noqa: E731
        None, None, None, None, N, None, B, L, E, None, None, None, eps, p, 4, 0, 0, None, None, None, None)
    bwd = lambda B, L, E, p, want, gp: lib.tbe_history_backward_f32(  # noqa: E731
        None, None, None, None, None, 0, None, B, L, E, None, None, None, p, 4, 0, 0, None, gp, want, None, 0, None)
    assert fwd(1, 0, 129, 256, 0.0, 1e-5) == -1 and b"unsupported" in lib.tbe_last_error()
    assert fwd(-1, 0, 8, 16, 0.0, 1e-5) == -1 and fwd(1, -1, 8, 16, 0.0, 1e-5) == -1
    assert fwd(1, 0, 8, 16, 1.0, 1e-5) == -1 and b"dropout" in lib.tbe_last_error()
    assert fwd(1, 0, 8, 16, -0.5, 1e-5) == -1 and fwd(1, 0, 8, 16, float("nan"), 1e-5) == -1
    assert fwd(0, 0, 8, 16, 0.0, float("inf")) == -1 and b"eps" in lib.tbe_last_error()
    assert fwd(1, 0, 8, 16, 0.0, 1e-5) == -1 and b"null pointer" in lib.tbe_last_error()
    assert fwd(0, 0, 8, 16, 0.0, 1e-5) == 0  # an empty batch launches nothing
    assert bwd(1, 8, 18, 0.0, 0, None) == -1 and bwd(1, 8, 16, 1.5, 0, None) == -1
    assert bwd(0, 8, 16, 0.0, 8, None) == -1 and b"want" in lib.tbe_last_error()
    assert bwd(0, 8, 16, 0.0, 7, None) == -1 and bwd(0, 8, 16, 0.0, 7, 4) == -1  # grad_params null, misaligned
    assert bwd(1, 8, 16, 0.0, 0, None) == -1 and b"null pointer" in lib.tbe_last_error()
    assert bwd(0, 8, 16, 0.0, 0, None) == 0
