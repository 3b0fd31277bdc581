"""The transform configuration surface (transform/transform_args.py, transform_scheme.py, transform_config.py upstream) as plain
dataclasses: same fields, same defaults, and `to_dict` / `model_dump` write exactly what upstream's pydantic `model_dump()`
writes into a checkpoint's config.json (`precision` as "torch.float32").  Duck-typed like quantization/quant_args.py: wherever
one of these is accepted, upstream's own pydantic object is accepted too (`coerce`)."""
from dataclasses import dataclass, field
from enum import Enum
from typing import Dict, List, Optional

import torch

__all__ = ["TransformLocation", "TransformArgs", "TransformScheme", "TransformConfig", "TRANSFORM_CONFIG_NAME"]

TRANSFORM_CONFIG_NAME = "transform_config"  # the model attribute and the config.json key (upstream base.py)


class TransformLocation(str, Enum):
    """transform_args.py:12-44"""

    INPUT = "input"
    WEIGHT_INPUT = "weight_input"
    WEIGHT_OUTPUT = "weight_output"
    OUTPUT = "output"
    K_CACHE = "k_cache"
    Q_ATTN = "q_attn"

    def is_online(self) -> bool:
        return self not in (TransformLocation.WEIGHT_INPUT, TransformLocation.WEIGHT_OUTPUT)


def _wrap(value) -> List[str]:
    return [value] if isinstance(value, str) else list(value)


def _dtype_of(value) -> torch.dtype:
    if isinstance(value, torch.dtype):
        return value
    name = str(value).removeprefix("torch.")
    dt = getattr(torch, name, None)
    if not isinstance(dt, torch.dtype):
        raise ValueError(f"unknown torch dtype {value!r}")
    return dt


def _check_keys(cls, d):
    extra = set(d) - set(cls.__dataclass_fields__)
    if extra:
        raise ValueError(f"{cls.__name__}: unexpected fields {sorted(extra)}")  # extra="forbid" upstream


@dataclass
class TransformArgs:
    """transform_args.py:47-73; `location` is kept as its string value (use_enum_values upstream)"""

    targets: List[str]
    location: str
    inverse: bool = False
    ignore: List[str] = field(default_factory=list)

    def __post_init__(self):
        self.targets = _wrap(self.targets)
        self.ignore = _wrap(self.ignore)
        self.location = TransformLocation(getattr(self.location, "value", self.location)).value

    def is_online(self) -> bool:
        return TransformLocation(self.location).is_online()

    def to_dict(self) -> dict:
        return {"targets": list(self.targets), "location": self.location, "inverse": bool(self.inverse), "ignore": list(self.ignore)}

    @classmethod
    def from_dict(cls, d: dict) -> "TransformArgs":
        _check_keys(cls, d)
        return cls(**d)

    @classmethod
    def coerce(cls, obj) -> "TransformArgs":
        if isinstance(obj, cls):
            return obj
        if isinstance(obj, dict):
            return cls.from_dict(obj)
        return cls(targets=obj.targets, location=obj.location, inverse=obj.inverse, ignore=obj.ignore)


@dataclass
class TransformScheme:
    """transform_scheme.py:13-42"""

    type: str
    apply: List[TransformArgs] = field(default_factory=list)
    randomize: bool = False
    requires_grad: bool = False
    head_dim: Optional[int] = None
    precision: torch.dtype = torch.float32

    def __post_init__(self):
        self.apply = [TransformArgs.coerce(a) for a in self.apply]
        self.precision = _dtype_of(self.precision)

    def to_dict(self) -> dict:
        return {"type": self.type, "apply": [a.to_dict() for a in self.apply], "randomize": bool(self.randomize),
                "requires_grad": bool(self.requires_grad), "head_dim": self.head_dim, "precision": str(self.precision)}

    @classmethod
    def from_dict(cls, d: dict) -> "TransformScheme":
        _check_keys(cls, d)
        return cls(**d)

    @classmethod
    def coerce(cls, obj) -> "TransformScheme":
        if isinstance(obj, cls):
            return obj
        if isinstance(obj, dict):
            return cls.from_dict(obj)
        return cls(type=obj.type, apply=list(obj.apply), randomize=obj.randomize, requires_grad=obj.requires_grad,
                   head_dim=obj.head_dim, precision=obj.precision)


@dataclass
class TransformConfig:
    """transform_config.py:12-32"""

    config_groups: Dict[str, TransformScheme]

    def __post_init__(self):
        self.config_groups = {k: TransformScheme.coerce(v) for k, v in self.config_groups.items()}

    def to_dict(self) -> dict:
        return {"config_groups": {k: v.to_dict() for k, v in self.config_groups.items()}}

    def model_dump(self, **kwargs) -> dict:
        """what ModelCompressor.update_config writes under "transform_config" (it calls model_dump where one exists)"""
        return self.to_dict()

    @classmethod
    def from_dict(cls, d: dict) -> "TransformConfig":
        _check_keys(cls, d)
        return cls(**d)

    @classmethod
    def coerce(cls, obj) -> "TransformConfig":
        if isinstance(obj, cls):
            return obj
        if isinstance(obj, dict):
            return cls.from_dict(obj)
        return cls(config_groups=dict(obj.config_groups))

    def merge(self, other) -> None:
        """config groups of `other` are appended under unique keys (transform_config.py:25-32)"""
        for key, scheme in TransformConfig.coerce(other).config_groups.items():
            unique, i = key, 0
            while unique in self.config_groups:
                i += 1
                unique = f"{key}_{i}"
            self.config_groups[unique] = scheme
