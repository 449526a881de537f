"""Helpers of the dense modules with the reference's contracts (torchrec/modules/utils.py)."""
from typing import Callable, Union

import torch


def extract_module_or_tensor_callable(
        module_or_callable: Union[Callable[[], torch.nn.Module], torch.nn.Module, Callable[[torch.Tensor], torch.Tensor]],
) -> Union[torch.nn.Module, Callable[[torch.Tensor], torch.Tensor]]:
    """What `MLP` hands each of its layers as the activation (torchrec/modules/utils.py:14-35): a zero-argument factory
    (`nn.ReLU`, a lambda) is called and its module returned, so that layers share no activation parameters; anything that
    needs a positional argument — a tensor function such as `torch.relu`, a module instance — comes back as the same
    object.  A factory that returns something other than an `nn.Module` raises ValueError; any other TypeError of the call
    propagates."""
    try:
        module = module_or_callable()
    except TypeError as e:
        if "required positional argument" in str(e):
            return module_or_callable
        raise
    if isinstance(module, torch.nn.Module):
        return module
    raise ValueError(f"Expected callable that takes no input to return a torch.nn.Module, but got: {type(module)}")
