"""apply_transform_config (transform/apply.py:14-30 with TransformFactory._apply_to_module, transform/factory/base.py:105-190)
for the deterministic `hadamard` type."""
import torch

from ..entrypoints.convert.converters import match_name
from .config import TRANSFORM_CONFIG_NAME, TransformConfig, TransformLocation
from .hadamard import HadamardTransform, get_transform_size

__all__ = ["apply_transform_config", "match_named_modules"]


def _match_class(module: torch.nn.Module, target: str) -> bool:
    """utils/match.py:448-465: the name of any torch.nn.Module parent class"""
    return any(issubclass(c, torch.nn.Module) and c.__name__ == target for c in type(module).__mro__)


def _is_match(name, module, targets) -> bool:
    return any(match_name(name, t) or _match_class(module, t) for t in targets)


def match_named_modules(model: torch.nn.Module, targets, ignore=()):
    """utils/match.py:34-64: (name, module) of every module a target matches and no ignore entry does, in named_modules order"""
    targets, ignore = list(targets or []), list(ignore or [])
    for name, module in model.named_modules():
        if isinstance(module, HadamardTransform):
            continue  # InternalModule upstream
        if _is_match(name, module, targets) and not _is_match(name, module, ignore):
            yield name, module


def _check_supported(name, scheme) -> None:
    if scheme.type != "hadamard":
        raise NotImplementedError(f"config group {name!r}: type={scheme.type!r} is not built here (only the deterministic 'hadamard' type is)")
    if scheme.randomize:
        raise NotImplementedError(f"config group {name!r}: randomize=True needs upstream's permutation, which is not built here")
    if scheme.requires_grad:
        raise NotImplementedError(f"config group {name!r}: requires_grad=True (training, parametrization) is not built here")
    for args in scheme.apply:
        if TransformLocation(args.location) in (TransformLocation.Q_ATTN, TransformLocation.K_CACHE):
            raise NotImplementedError(f"config group {name!r}: location={args.location!r} needs attention / KV-cache hooks, which are not built here")


def _apply_to_module(name, scheme, module, args) -> None:
    location = TransformLocation(args.location)
    transform = HadamardTransform(get_transform_size(module, location, scheme.head_dim), scheme, args, type(module))
    transform_name = f"{name}_{location.value}"
    if location == TransformLocation.INPUT:
        module.register_module(transform_name, transform)
        module.register_forward_pre_hook(lambda _, inputs: transform(inputs[0]), prepend=True)
    elif location == TransformLocation.OUTPUT:
        module.register_module(transform_name, transform)
        module.register_forward_hook(lambda _, _inputs, output: transform(output))
    else:
        assert hasattr(module, "weight")
        with torch.no_grad():
            module.weight.copy_(transform(module.weight))
            # y' = R (W x + b) = (R W) x + R b: the bias rotates with the output side (base.py:137-146)
            if location == TransformLocation.WEIGHT_OUTPUT and getattr(module, "bias", None) is not None:
                module.bias.copy_(transform(module.bias.unsqueeze(-1)).squeeze(-1))


def apply_transform_config(model: torch.nn.Module, config) -> None:
    """Weight locations are fused into the weights (and the bias, for weight_output) under no_grad; `input` becomes a prepended
    forward pre-hook and `output` a forward hook on a HadamardTransform submodule.  `config` (ours or upstream's pydantic
    object) is attached to the model as `transform_config`, where ModelCompressor.from_pretrained_model picks it up.  Everything
    is checked before anything is changed: q_attn / k_cache, requires_grad, randomize and every type but "hadamard" raise
    NotImplementedError naming the field."""
    ours = TransformConfig.coerce(config)
    for name, scheme in ours.config_groups.items():
        _check_supported(name, scheme)
    for name, scheme in ours.config_groups.items():
        for args in scheme.apply:
            for _, module in list(match_named_modules(model, args.targets, args.ignore)):
                _apply_to_module(name, scheme, module, args)
    setattr(model, TRANSFORM_CONFIG_NAME, config)
