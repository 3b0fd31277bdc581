"""HadamardTransform (transform/factory/hadamard.py:72-108) for the deterministic Sylvester matrix, on the fast Walsh-Hadamard
kernels of csrc/ct_hadamard.hip: the module holds a size, not an n x n weight."""
import torch

from .. import codec
from .config import TransformArgs, TransformLocation, TransformScheme

__all__ = ["HadamardTransform", "get_transform_size", "transform_dim"]


def get_transform_size(module: torch.nn.Module, location, head_dim=None) -> int:
    """transform/utils/matrix.py:11-49"""
    location = TransformLocation(getattr(location, "value", location))
    size = None
    if isinstance(module, torch.nn.Linear):
        size = module.in_features if location in (TransformLocation.INPUT, TransformLocation.WEIGHT_INPUT) else module.out_features
    elif isinstance(module, torch.nn.Embedding):
        size = module.num_embeddings if location in (TransformLocation.INPUT, TransformLocation.WEIGHT_INPUT) else module.embedding_dim
    elif head_dim is None:
        raise NotImplementedError(f"Transforms on {type(module)} are not supported without head_dim")
    if head_dim is not None:
        if size is not None and size % head_dim != 0:
            raise ValueError(f"{head_dim} must divide {size} for {type(module)} at {location}")
        size = head_dim
    return size


def transform_dim(location, module_type) -> int:
    """the dimension apply_transform_weight (transform/utils/matrix.py:97-121) multiplies along: the last one for the online
    locations, Linear weight_input (W @ H.T) and Embedding weight_output (W @ H); dim 0 for Linear weight_output (H.T @ W) and
    Embedding weight_input (H @ W)"""
    location = TransformLocation(getattr(location, "value", location))
    if location.is_online():
        return -1
    if module_type is not None and issubclass(module_type, torch.nn.Linear):
        return -1 if location == TransformLocation.WEIGHT_INPUT else 0
    if module_type is not None and issubclass(module_type, torch.nn.Embedding):
        return 0 if location == TransformLocation.WEIGHT_INPUT else -1
    raise NotImplementedError(f"Applying transforms to {module_type} {location} is not supported")


class HadamardTransform(torch.nn.Module):
    """value -> value rotated by H_size / sqrt(size) at `args.location` of a module of `module_type`.  Fused (offline) locations
    accumulate in float64, online ones in `scheme.precision` (hadamard.py:44).  The Sylvester matrix is symmetric, so
    `args.inverse` selects the same rotation."""

    def __init__(self, size: int, scheme, args, module_type=torch.nn.Linear):
        super().__init__()
        self.size = int(size)
        self.scheme = TransformScheme.coerce(scheme)
        self.args = TransformArgs.coerce(args)
        self.module_type = module_type
        self.dim = transform_dim(self.args.location, module_type)
        self.precision = self.scheme.precision if self.args.is_online() else torch.float64

    def forward(self, value: torch.Tensor) -> torch.Tensor:
        return codec.hadamard_transform(value.contiguous(), self.size, dim=self.dim, precision=self.precision)

    def right_inverse(self, value: torch.Tensor) -> torch.Tensor:
        return self.forward(value)

    def extra_repr(self) -> str:
        return f"size={self.size}, location={self.args.location}, inverse={self.args.inverse}, precision={self.precision}"
