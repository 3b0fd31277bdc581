"""The `random-hadamard` transform (transform/factory/random_hadamard.py) on the kernels of csrc/ct_hadamard_k.hip.

`random_hadamard_matrix(n)` (transform/utils/hadamard.py:53-151) is W = diag(s) * (hadK (x) H_M)^T: s the drawn +-1 vector, hadK
the known K x K Hadamard matrix of the largest K with M = n / K a power of two, H_M the Sylvester matrix in natural order.  The
table of known matrices is upstream's data and is not shipped: `factor_hadamard_weight` recovers (K, M, hadK, s) from a given W,
and `RandomHadamardTransform` holds those factors — n + K^2 bytes instead of the 4 n^2 of the weight."""
from typing import NamedTuple, Optional

import torch

from .. import codec
from .config import TransformArgs, TransformLocation, TransformScheme
from .hadamard import _PermutedMixin, transform_dim

__all__ = ["HadamardFactors", "factor_hadamard_weight", "RandomHadamardTransform", "transform_transposed"]


class HadamardFactors(NamedTuple):
    n: int
    k: int
    m: int
    had_k: Optional[torch.Tensor]  # int8 (k, k), None when k == 1 (the Sylvester part covers everything)
    signs: torch.Tensor  # int8 (n,)


def _sylvester(m: int, device) -> torch.Tensor:
    """H_m in natural order as int8: (-1)^popcount(i & j)"""
    i = torch.arange(m, device=device)
    bits = i[:, None] & i[None, :]
    parity = torch.zeros_like(bits)
    while bool(bits.any()):
        parity ^= bits & 1
        bits = bits >> 1
    return (1 - 2 * parity).to(torch.int8)


def _matches(w: torch.Tensor, signs: torch.Tensor, had_k: torch.Tensor, m: int) -> bool:
    """W == signs[:, None] * kron(had_k, H_m).T, checked a block row at a time (no second n x n tensor)"""
    k = had_k.shape[0]
    h = _sylvester(m, w.device)
    w4 = w.view(k, m, k, m)  # W[(a, t), (b, u)] = signs[(a, t)] * had_k[b, a] * H_m[u, t]
    s2 = signs.view(k, m)
    for a in range(k):
        want = s2[a].view(m, 1, 1) * had_k[:, a].view(1, k, 1) * h.t().reshape(m, 1, m)
        if not torch.equal(w4[a], want):
            return False
    return True


def factor_hadamard_weight(weight: torch.Tensor) -> Optional[HadamardFactors]:
    """(n, k, m, had_k, signs) with weight == signs[:, None] * kron(had_k, H_m).T for the LARGEST power of two m dividing n for
    which that holds, or None when the weight is not square, not +-1, or not a Hadamard matrix (m == 1 always reconstructs a +-1
    weight — had_k is then the weight with row 0's signs moved into `signs` — so the rows of had_k are checked for orthogonality).
    signs = weight[:, 0]; had_k[b, a] = weight[a m, 0] * weight[a m, b m] — row 0's signs are absorbed.  had_k is dropped (k
    becomes 1) when m == n, the pure Sylvester case.  Runs on the weight's device."""
    if weight.dim() != 2 or weight.shape[0] != weight.shape[1] or weight.shape[0] == 0:
        return None
    n = int(weight.shape[0])
    w = weight.detach().to(torch.int8)
    if not bool(((w == 1) | (w == -1)).all()) or not torch.equal(w.to(weight.dtype), weight.detach()):
        return None
    signs = w[:, 0].contiguous()
    m = n & -n  # the largest power of two dividing n
    while m >= 1:
        k = n // m
        had_k = (w[::m, 0].view(1, k) * w[::m, ::m].t()).contiguous()  # [b, a] = W[a m, 0] * W[a m, b m]
        if _matches(w, signs, had_k, m):
            f = had_k.to(torch.float32)  # +-1 entries, sums below 2^24: exact
            if not torch.equal(f @ f.t(), k * torch.eye(k, device=w.device)):
                return None  # +-1 but not a Hadamard matrix: the rows are not orthogonal
            return HadamardFactors(n, k, m, None if k == 1 else had_k, signs)
        m //= 2
    return None


def transform_transposed(location, module_type, inverse: bool) -> bool:
    """whether apply_transform_weight (transform/utils/matrix.py:97-121) multiplies the transformed dimension by W.T (True) or by
    W (False): W for the online locations, Embedding weight_output and Linear weight_output (W.T @ value: columns times W), W.T
    for Linear weight_input (value @ W.T) and Embedding weight_input (W @ value).  `inverse` transposes the weight first
    (transform/factory/hadamard.py:97-98) and so selects the other form."""
    location = TransformLocation(getattr(location, "value", location))
    return (location == TransformLocation.WEIGHT_INPUT) != bool(inverse)


class RandomHadamardTransform(_PermutedMixin, torch.nn.Module):
    """value -> value @ W / sqrt(n) (or W.T, per location, module type and `args.inverse`) for a factored random-hadamard weight.
    Fused (offline) locations accumulate in float64, online ones in `scheme.precision`, as HadamardTransform does.  Not a
    HadamardTransform: fuse_input_quantization, which fuses the Sylvester rotation into the QDQ launch, leaves it alone.
    `perm` (randomize=True upstream): the weight W[perm][:, perm]."""

    def __init__(self, factors: HadamardFactors, scheme, args, module_type=torch.nn.Linear, perm=None):
        super().__init__()
        self.size, self.k, self.m = int(factors.n), int(factors.k), int(factors.m)
        self.register_buffer("had_k", factors.had_k, persistent=False)
        self.register_buffer("signs", factors.signs, persistent=False)
        self.scheme = TransformScheme.coerce(scheme)
        self.args = TransformArgs.coerce(args)
        self.module_type = module_type
        self.dim = transform_dim(self.args.location, module_type)
        self.transposed = transform_transposed(self.args.location, module_type, self.args.inverse)
        self.precision = self.scheme.precision if self.args.is_online() else torch.float64
        self._init_perm(perm, self.size)

    def forward(self, value: torch.Tensor) -> torch.Tensor:
        if self.perm is None:
            return codec.hadamard_k_transform(value.contiguous(), self.size, self.had_k, self.signs, dim=self.dim, precision=self.precision,
                                              transposed=self.transposed)
        return codec.hadamard_k_transform(value.contiguous(), self.size, self.had_k, self.signs, dim=self.dim, precision=self.precision,
                                          transposed=self.transposed, perm=self.perm_tables(value.device))

    def extra_repr(self) -> str:
        return (f"size={self.size} ({self.k} x {self.m}), location={self.args.location}, inverse={self.args.inverse}, "
                f"transposed={self.transposed}, precision={self.precision}, permuted={self.perm is not None}")
