"""CPU: the support rule of the tiled attention kernels (csrc/attention_tiled.hip) and their argument checks, which come
before any launch and need no device."""
import pytest

import _paths  # noqa: F401
from fbgemm_gpu import _lib


@pytest.mark.parametrize("L, d, inside", [(200, 128, True), (257, 4, True), (4096, 128, True), (1, 4, True),
                                          (4097, 4, False), (8, 6, False), (8, 132, False), (0, 8, False)])
def test_support_rule(L, d, inside):
    assert bool(_lib.load().tbe_attention_tiled_supported(L, d)) == inside


def test_a_null_q_is_refused_before_any_launch():
    lib = _lib.load()
    qkv = [None, 64, 8] * 3
    assert lib.tbe_attention_tiled_forward_f32(*qkv, None, 1, 1, 8, 8, 0.0, 0, 0, None, None, None) == -1
    assert b"tbe_attention_tiled_forward_f32" in lib.tbe_last_error()
    assert lib.tbe_attention_tiled_backward_f32(None, None, *qkv, None, None, 1, 1, 8, 8, 0.0, 0, 0, None, None, None, None,
                                                None) == -1
    assert b"tbe_attention_tiled_backward_f32" in lib.tbe_last_error()
