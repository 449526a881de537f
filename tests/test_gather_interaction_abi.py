"""CPU: the two gather-interaction entry points (include/tbe_hip.h) are exported and refuse bad arguments before any
launch."""
import _paths  # noqa: F401
from fbgemm_gpu import _lib

FWD = "tbe_dlrm_interaction_gather_forward_f32"
BWD = "tbe_dlrm_interaction_gather_backward_f32"


def test_gather_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name in (FWD, BWD):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.tbe_abi_version() == 3


def _fwd(lib, B=4, F=26, D=128, stride=479, ptr=16):
    return lib.tbe_dlrm_interaction_gather_forward_f32(ptr, ptr, ptr, None, ptr, B, F, D, ptr, stride, None, None)


def _bwd(lib, B=4, F=26, D=128, stride=479, ptr=16):
    return lib.tbe_dlrm_interaction_gather_backward_f32(ptr, ptr, ptr, None, ptr, ptr, stride, B, F, D, ptr, ptr, None, None)


def test_gather_entry_points_validate_before_any_launch():
    lib = _lib.load()
    for call in (_fwd, _bwd):
        assert call(lib, F=28) == -1 and b"F=28" in lib.tbe_last_error()
        assert call(lib, F=0) == -1
        assert call(lib, D=48) == -1 and b"D=48" in lib.tbe_last_error()
        assert call(lib, stride=478) == -1 and b"stride" in lib.tbe_last_error()
        assert call(lib, ptr=None) == -1 and b"null pointer" in lib.tbe_last_error()
        assert call(lib, ptr=20) == -1 and b"aligned" in lib.tbe_last_error()
        assert call(lib, B=0) == 0  # an empty batch launches nothing
