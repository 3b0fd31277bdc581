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


class _PermutedMixin:
    """the permutation of `randomize=True` on a transform: `perm` is a persistent int64 buffer (upstream's state_dict key
    `<name>_<location>.perm`: the draw cannot be regenerated); its device tables (codec.hadamard_perm_tables) are built once per
    device and rebuilt when the buffer is replaced or written"""

    def _init_perm(self, perm, size):
        if perm is not None:
            perm = torch.as_tensor(perm).detach().to(torch.int64)
            codec.hadamard_perm_tables(perm, "cpu")  # validates; the device tables come with the first call
            if perm.numel() != size:
                raise ValueError(f"the permutation has {perm.numel()} entries, the rotation size is {size}")
        self.register_buffer("perm", perm, persistent=True)
        self._perm_tables = {}

    def perm_tables(self, device):
        """None for an unpermuted transform"""
        if self.perm is None:
            return None
        device = torch.device(device)
        key = (self.perm._version, self.perm.data_ptr())
        hit = self._perm_tables.get(device)
        if hit is None or hit[0] != key:
            hit = self._perm_tables[device] = (key, codec.hadamard_perm_tables(self.perm, device))
        return hit[1]


class HadamardTransform(_PermutedMixin, torch.nn.Module):
    """value -> value rotated by H_size / sqrt(size) at `args.location` of a module of `module_type`.  Fused (offline) locations
    accumulate in float64, online ones in `scheme.precision` (hadamard.py:44).  The Sylvester matrix is symmetric, so
    `args.inverse` selects the same rotation.  `perm` (randomize=True upstream): the matrix H[perm][:, perm], still symmetric."""

    def __init__(self, size: int, scheme, args, module_type=torch.nn.Linear, perm=None):
        super().__init__()
        self.size = int(size)
        self.scheme = TransformScheme.coerce(scheme)
        self.args = TransformArgs.coerce(args)
        self.module_type = module_type
        self.dim = transform_dim(self.args.location, module_type)
        self.precision = self.scheme.precision if self.args.is_online() else torch.float64
        self._init_perm(perm, self.size)

    def forward(self, value: torch.Tensor) -> torch.Tensor:
        if self.perm is None:
            return codec.hadamard_transform(value.contiguous(), self.size, dim=self.dim, precision=self.precision)
        return codec.hadamard_transform(value.contiguous(), self.size, dim=self.dim, precision=self.precision, perm=self.perm_tables(value.device))

    def right_inverse(self, value: torch.Tensor) -> torch.Tensor:
        return self.forward(value)

    def extra_repr(self) -> str:
        return (f"size={self.size}, location={self.args.location}, inverse={self.args.inverse}, precision={self.precision}, "
                f"permuted={self.perm is not None}")
