"""CPU: tbe_dlrm_interaction_gather_forward_nbit (include/tbe_hip.h) is exported, bound, and refuses bad arguments before
any launch."""
import _paths  # noqa: F401
from fbgemm_gpu import _lib

NAME = "tbe_dlrm_interaction_gather_forward_nbit"


def _call(lib, bits=4, B=4, F=26, D=128, stride=479, ptr=16, dense=None, feat=None, ids=None):
    dense, feat, ids = (ptr if p is None else p for p in (dense, feat, ids))
    return getattr(lib, NAME)(dense, feat, feat, feat, bits, ids, B, F, D, ptr, stride, None, None)


def test_entry_is_exported_and_validates_before_any_launch():
    lib = _lib.load()
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES and lib.tbe_abi_version() == 3
    for kwargs, message in (
            (dict(F=0), b"F=0 outside"), (dict(F=28, stride=1 << 20), b"F=28 outside"), (dict(D=32), b"D=32 not in"),
            (dict(D=256, stride=1 << 20), b"D=256 not in"), (dict(bits=16), b"bit_rate=16"), (dict(bits=0), b"bit_rate=0"),
            (dict(stride=478), b"stride 478 <"), (dict(ptr=None), b"null pointer"), (dict(feat=0), b"null pointer"),
            (dict(ids=0), b"null pointer"), (dict(dense=24), b"16-B aligned"), (dict(ids=20), b"8-B aligned"),
            (dict(feat=20), b"8-B"), (dict(ptr=18, dense=16, feat=16, ids=16), b"4-B aligned"), (dict(B=-1), b"outside")):
        assert _call(lib, **kwargs) == -1 and message in lib.tbe_last_error(), kwargs
    assert _call(lib, B=0) == 0  # an empty batch launches nothing
