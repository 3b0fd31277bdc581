"""apply_transform_config (transform/apply.py:14-30 with TransformFactory._apply_to_module, transform/factory/base.py:105-190)
for the deterministic `hadamard` type and, given the caller's matrix constructor, the `random-hadamard` type; and the opt-in `fuse_input_quantization`: an `input` rotation in front of a dynamically
quantized module runs in the QDQ's launch (csrc/ct_rotated.hip).  The `q_attn` / `k_cache` locations of a transformers model become
query / key hooks of modeling/ (base.py:167-189); the opt-in `fuse_attention_quantization` runs them in the launch of the static
q / k / v QDQ that follows (csrc/ct_attn_rot.hip)."""
import torch

from ..entrypoints.convert.converters import match_name
from ..modeling import (IMPL_ATTR, KV_CACHE_ATTR, QuantizedAttentionImpl, QuantizedKVCache, initialize_hooked_attention, initialize_hooked_kv_cache,
                        register_key_value_hook, register_query_hook)
from .config import TRANSFORM_CONFIG_NAME, TransformConfig, TransformLocation
from .hadamard import HadamardTransform, get_transform_size
from .random_hadamard import RandomHadamardTransform, factor_hadamard_weight

__all__ = ["apply_transform_config", "fuse_input_quantization", "fuse_attention_quantization", "match_named_modules"]


def _match_class(module: torch.nn.Module, target: str) -> bool:
    """utils/match.py:448-465: the name of any torch.nn.Module parent class"""
    return any(issubclass(c, torch.nn.Module) and c.__name__ == target for c in type(module).__mro__)


def _is_match(name, module, targets) -> bool:
    return any(match_name(name, t) or _match_class(module, t) for t in targets)


def match_named_modules(model: torch.nn.Module, targets, ignore=()):
    """utils/match.py:34-64: (name, module) of every module a target matches and no ignore entry does, in named_modules order"""
    targets, ignore = list(targets or []), list(ignore or [])
    for name, module in model.named_modules():
        if isinstance(module, (HadamardTransform, RandomHadamardTransform, QuantizedAttentionImpl, QuantizedKVCache)):
            continue  # InternalModule upstream
        if _is_match(name, module, targets) and not _is_match(name, module, ignore):
            yield name, module


_ATTENTION_LOCATIONS = (TransformLocation.Q_ATTN, TransformLocation.K_CACHE)


class AttentionHookError(ValueError, NotImplementedError):
    """upstream's `ValueError("Cannot hook attention of model: ...")` (base.py:169-170,180-181) for a q_attn / k_cache location on
    something that is not a transformers PreTrainedModel.  Also a NotImplementedError: that is what these locations raised before
    the hooks existed, and what callers that hand undone work to upstream catch."""


def _is_pretrained_model(model) -> bool:
    try:
        from transformers import PreTrainedModel
    except ImportError:
        return False
    return isinstance(model, PreTrainedModel)


def _check_supported(name, scheme, random_hadamard: bool = False, model=None, randomize: bool = False) -> None:
    if scheme.type != "hadamard" and not (random_hadamard and scheme.type == "random-hadamard"):
        raise NotImplementedError(f"config group {name!r}: type={scheme.type!r} is not built here (only the deterministic 'hadamard' type is)")
    if scheme.randomize and not randomize:
        raise NotImplementedError(f"config group {name!r}: randomize=True needs upstream's permutation, which is not built here")
    if scheme.requires_grad:
        raise NotImplementedError(f"config group {name!r}: requires_grad=True (training, parametrization) is not built here")
    for args in scheme.apply:
        if TransformLocation(args.location) in _ATTENTION_LOCATIONS and not _is_pretrained_model(model):
            raise AttentionHookError(f"config group {name!r}: location={args.location!r}: Cannot hook attention of model: {model}")


_INPUT_ROTATIONS = "_ct_input_rotations"  # module attribute: the InputRotation pre-hooks apply_transform_config registered


class InputRotation:
    """the forward pre-hook of an `input` transform: inputs[0] rotated.  With `fuse_quantization` set (fuse_input_quantization)
    and upstream's quantized_forward predicate true for the module, a call whose plan fuses returns the rotated AND dynamically
    quantized input from one launch and leaves a weak reference to it on the module; dynamic.forward_quantize(module, value,
    "input", args) hands that very tensor back untouched.  Every other call rotates only, as without the opt-in.
    Precondition of the opt-in: the module's forward calls forward_quantize(module, x, "input", ...) under that same predicate
    (upstream's quantized_forward does).  A module that carries a scheme and a status but runs a plain forward would receive a
    quantized input where it received a rotated one before — do not opt such a model in."""

    def __init__(self, transform: HadamardTransform):
        self.transform = transform
        self.fuse_quantization = False

    def __call__(self, module, inputs):
        value = inputs[0]
        if self.fuse_quantization:
            out = self._rotate_and_quantize(module, value)
            if out is not None:
                return out
        return self.transform(value)

    def _rotate_and_quantize(self, module, value):
        from ..quantization import dynamic

        scheme = getattr(module, "quantization_scheme", None)
        # quantized_forward's own predicate (quantization/lifecycle/forward.py:265-276)
        if not getattr(module, "quantization_enabled", True) or scheme is None or getattr(module, "quantization_status", None) is None:
            return None
        args = getattr(scheme, "input_activations", None)
        if args is None or not _dynamic_args(args, module) or self.transform.precision is not torch.float32 or self.transform.dim != -1:
            return None
        if self.transform.perm is not None:
            return None  # the fused launch rotates by size alone: it would drop the permutation
        value = value.contiguous()
        global_scale = getattr(module, "input_global_scale", None)
        try:
            if not dynamic.plan_rotated_dynamic(value.shape, value.dtype, self.transform.size, args, global_scale).fused:
                return None
        except (NotImplementedError, ValueError):
            return None  # the rotation alone raises what it raises
        if value.data_ptr() % 16:
            return None
        out = dynamic.rotated_fake_quantize(value, self.transform.size, args, global_scale)
        dynamic.remember_prequantized(module, out)
        return out


def _dynamic_args(args, module) -> bool:
    """a dynamic scheme of a kind plan_dynamic knows, on a module forward_quantize does not decline"""
    from ..quantization import dynamic

    if dynamic.enum_value(getattr(args, "dynamic", False)) not in (True, "local"):
        return False
    try:
        dynamic._kind(args, getattr(module, "input_global_scale", None))
    except NotImplementedError:
        return False
    if dynamic._g_idx_initialised(getattr(module, "weight_g_idx", None)) and dynamic.enum_value(args.strategy) in ("group", "tensor_group"):
        return False
    return True


def fuse_input_quantization(model: torch.nn.Module) -> list:
    """Opt-in, after apply_transform_config and after the quantization schemes are attached: every module whose ONE `input`
    HadamardTransform stands in front of dynamic `input_activations` of a kind the kernels know gets the fused pre-hook
    (InputRotation).  Returns the names of the modules it fused.  The model computes the same bits, one launch per fused module
    input instead of two; modules that do not qualify, and calls whose plan does not fuse, run as before.  Only for models whose
    quantized modules run a forward that calls forward_quantize on the input (set_forward_quantized): see InputRotation."""
    fused = []
    for name, module in model.named_modules():
        hooks = module.__dict__.get(_INPUT_ROTATIONS, ())
        args = getattr(getattr(module, "quantization_scheme", None), "input_activations", None)
        if len(hooks) != 1 or args is None or not _dynamic_args(args, module) or hooks[0].transform.perm is not None:
            continue  # a permuted rotation has no fused launch; several rotations: only the last one could share the QDQ's launch, and the hooks do not know their order
        hooks[0].fuse_quantization = True
        fused.append(name)
    return fused


_ATTN_ROTATIONS = "_ct_attn_rotations"  # attention-module attribute: {"q": QueryRotation, "k": KeyRotation} of apply_transform_config


def _static_attn_args(module, base_names):
    """the predicate of the consumer (QuantizedAttentionImpl / QuantizedKVCache.forward, then forward_quantize's strided branch):
    the module's static tensor / attn_head input_activations with every state's scale on the module and no global scale, or None"""
    from ..quantization import dynamic

    args = getattr(getattr(module, "quantization_scheme", None), "input_activations", None)
    if args is None or not getattr(module, "quantization_enabled", True):
        return None
    if dynamic.enum_value(getattr(args, "dynamic", False)) in (True, "local") or dynamic.enum_value(args.strategy) not in ("tensor", "attn_head"):
        return None
    for b in base_names:
        if getattr(module, f"{b}_scale", None) is None or getattr(module, f"{b}_global_scale", None) is not None:
            return None
    return args


class _AttentionRotation:
    """a `q_attn` / `k_cache` transform as a named hook.  `handle` is its forward pre-hook on the module's impl / kv_cache.  With
    `fuse_quantization` set (fuse_attention_quantization), a call for which the consumer's own predicate holds — static tensor /
    attn_head `input_activations`, quantization enabled, scales on the module, no global scales, GPU states — and whose plan fuses
    returns the rotated AND quantized states from one launch (csrc/ct_attn_rot.hip) and leaves weak references to them on the
    attention module; forward_quantize / quantize_key_value hand those very tensors back untouched.  Every other call rotates
    only, as without the opt-in.
    Precondition of the opt-in: this hook is the last pre-hook of the impl / cache, and stays the last.  A hook registered on
    the impl or the cache AFTER opting in would see quantized states where it saw rotated ones before (a hook that REPLACES a
    state is safe: the replacement is another tensor, and is quantized as always)."""

    def __init__(self, transform):
        self.transform = transform
        self.fuse_quantization = False
        self.handle = None

    def fusable(self) -> bool:
        return (isinstance(self.transform, HadamardTransform) and self.transform.perm is None  # the fused launch would drop a permutation
                and self.transform.precision is torch.float32 and self.transform.dim == -1)

    def _kw(self, args):
        from ..quantization import dynamic

        return dict(num_bits=int(args.num_bits), strategy=dynamic.enum_value(args.strategy), qtype=dynamic.enum_value(getattr(args, "type", "int")))


class QueryRotation(_AttentionRotation):
    """the query hook of a `q_attn` transform (see _AttentionRotation): hand-off under base name "q" """

    def __call__(self, module, query_states):
        if self.fuse_quantization:
            out = self._rotate_and_quantize(module, query_states)
            if out is not None:
                return out
        return self.transform(query_states)

    def _rotate_and_quantize(self, module, value):
        from .. import codec
        from ..quantization import dynamic

        args = _static_attn_args(module, ("q",)) if self.fusable() else None
        if args is None or not codec.ATTN_ROTATED_MEASURED_FASTER["single"]:
            return None
        scale = module.q_scale
        try:
            if not codec._attn_rot_fusable(value, self.transform.size, scale, args.strategy, scale.dtype):
                return None
            out = codec.attn_rotated_fake_quantize(value, self.transform.size, scale, getattr(module, "q_zero_point", None), fused=True, **self._kw(args))
        except (NotImplementedError, ValueError):
            return None  # the rotation alone raises what it raises
        dynamic.remember_prequantized(module, out, "q")
        return out


class KeyRotation(_AttentionRotation):
    """the key hook of a `k_cache` transform (see _AttentionRotation): it sees both states of a cache update; fused, K is rotated
    and quantized and V quantized in ONE launch, handed off under "k" and "v" """

    def __call__(self, module, key_states, value_states):
        if self.fuse_quantization:
            out = self._rotate_and_quantize(module, key_states, value_states)
            if out is not None:
                return out
        return self.transform(key_states), value_states

    def _rotate_and_quantize(self, module, key_states, value_states):
        from .. import codec
        from ..modeling.kvcache import _static_pair_args
        from ..quantization import dynamic

        args = _static_attn_args(module, ("k", "v")) if self.fusable() else None
        if args is None or not codec.ATTN_ROTATED_MEASURED_FASTER["pair"] or not _static_pair_args(module, key_states, value_states, args):
            return None
        ks, vs = module.k_scale, module.v_scale
        try:
            if not codec._attn_rot_pair_fusable(key_states, value_states, self.transform.size, ks, vs, args.strategy):
                return None
            k, v = codec.attn_rotated_fake_quantize_pair(key_states, value_states, self.transform.size, ks, vs, getattr(module, "k_zero_point", None),
                                                         getattr(module, "v_zero_point", None), fused=True, **self._kw(args))
        except (NotImplementedError, ValueError):
            return None
        dynamic.remember_prequantized(module, k, "k")
        dynamic.remember_prequantized(module, v, "v")
        return k, v


def fuse_attention_quantization(model: torch.nn.Module) -> list:
    """Opt-in, after apply_transform_config and after the quantization schemes are attached, the sibling of
    fuse_input_quantization: every attention module with a deterministic float32 HadamardTransform at `q_attn` and / or `k_cache`
    whose rotation hook is the LAST forward pre-hook of its impl / kv_cache gets the fused hooks (QueryRotation, KeyRotation).
    Returns the names of the modules it fused (one entry per module, whichever of its rotations qualified).  The model computes
    the same bits: one launch for the query states and one for K + V where there were three and four — for the calls
    modeling.ROTATED_MEASURED_FASTER dispatches; every other call rotates only, as before.  `random-hadamard` rotations are left
    alone.  Hooks registered on the impl or the cache after opting in would see quantized states: see _AttentionRotation."""
    fused = []
    for name, module in model.named_modules():
        hit = False
        for key, owner_attr in (("q", IMPL_ATTR), ("k", KV_CACHE_ATTR)):
            hook = module.__dict__.get(_ATTN_ROTATIONS, {}).get(key)
            owner = getattr(module, owner_attr, None)
            if hook is None or owner is None or not hook.fusable() or hook.handle is None:
                continue
            order = list(owner._forward_pre_hooks)
            if not order or order[-1] != hook.handle.id:
                continue  # a later hook would see quantized states where it saw rotated ones
            hook.fuse_quantization = True
            hit = True
        if hit:
            fused.append(name)
    return fused


class _RandomWeights:
    """the weights of one `random-hadamard` config group, as RandomHadamardFactory keeps them: one generator per group (unseeded,
    as TransformFactory.__init__ leaves it without a seed), one draw per size in order of first use (ParameterizedDefaultDict keys
    the cache by size alone), drawn at the precision of that first use — and factored once"""

    def __init__(self, name, hadamard_weights, seed=None):
        self.name, self.hadamard_weights = name, hadamard_weights
        self.generator = torch.Generator()
        if seed is not None:  # TransformFactory.__init__: `if seed is not None: self.generator.manual_seed(seed)`
            self.generator.manual_seed(seed)
        self.factors = {}

    def get(self, size, precision, device):
        if size not in self.factors:
            weight = self.hadamard_weights(size, precision, device, self.generator)
            factors = factor_hadamard_weight(weight)
            if factors is None:
                raise ValueError(f"config group {self.name!r}: the weight of size {size} is not signs * kron(hadK, Sylvester).T")
            self.factors[size] = factors
        return self.factors[size]


class _Permutations:
    """the permutations of one config group with randomize=True, as HadamardFactory keeps them (transform/factory/hadamard.py:53,
    67-69): a CPU int64 `torch.randperm(size, generator=g)` per size, drawn at first use from the group's generator and shared by
    every transform of that size, online or offline"""

    def __init__(self, generator):
        self.generator = generator
        self.perms = {}

    def get(self, size):
        if size not in self.perms:
            self.perms[size] = torch.randperm(size, generator=self.generator)
        return self.perms[size]


def _apply_to_module(name, scheme, module, args, random_weights=None, model=None, perms=None) -> None:
    location = TransformLocation(args.location)
    size = get_transform_size(module, location, scheme.head_dim)
    if scheme.type == "random-hadamard":
        device = next((p.device for p in module.parameters()), torch.device("cpu"))
        factors = random_weights.get(size, scheme.precision if location.is_online() else torch.float64, device)
        perm = perms.get(size) if perms is not None else None  # after that size's weight, from the same generator
        transform = RandomHadamardTransform(factors, scheme, args, type(module), perm=perm)
    else:
        transform = HadamardTransform(size, scheme, args, type(module), perm=perms.get(size) if perms is not None else None)
    transform_name = f"{name}_{location.value}"
    if location == TransformLocation.INPUT:
        module.register_module(transform_name, transform)
        if isinstance(transform, HadamardTransform):
            hook = InputRotation(transform)
            module.__dict__.setdefault(_INPUT_ROTATIONS, []).append(hook)
        else:
            def hook(_, inputs, transform=transform):
                return transform(inputs[0])
        module.register_forward_pre_hook(hook, prepend=True)
    elif location == TransformLocation.OUTPUT:
        module.register_module(transform_name, transform)
        module.register_forward_hook(lambda _, _inputs, output: transform(output))
    elif location == TransformLocation.Q_ATTN:
        # the post-rope query states, rotated over the head dimension before they are quantized (base.py:167-176)
        module.register_module(transform_name, transform)
        initialize_hooked_attention(model, module)
        hook = QueryRotation(transform)
        hook.handle = register_query_hook(module, hook)
        module.__dict__.setdefault(_ATTN_ROTATIONS, {})["q"] = hook  # the last one registered: the one that can share the QDQ's launch
    elif location == TransformLocation.K_CACHE:
        module.register_module(transform_name, transform)
        initialize_hooked_kv_cache(model, module)
        hook = KeyRotation(transform)
        hook.handle = register_key_value_hook(module, hook)
        module.__dict__.setdefault(_ATTN_ROTATIONS, {})["k"] = hook
    else:
        assert hasattr(module, "weight")
        with torch.no_grad():
            module.weight.copy_(transform(module.weight))
            # y' = R (W x + b) = (R W) x + R b: the bias rotates with the output side (base.py:137-146)
            if location == TransformLocation.WEIGHT_OUTPUT and getattr(module, "bias", None) is not None:
                module.bias.copy_(transform(module.bias.unsqueeze(-1)).squeeze(-1))


def apply_transform_config(model: torch.nn.Module, config, *, hadamard_weights=None, randomize: bool = False, seed=None) -> None:
    """Weight locations are fused into the weights (and the bias, for weight_output) under no_grad; `input` becomes a prepended
    forward pre-hook and `output` a forward hook on a HadamardTransform submodule.  `config` (ours or upstream's pydantic
    object) is attached to the model as `transform_config`, where ModelCompressor.from_pretrained_model picks it up.  Everything
    is checked before anything is changed: requires_grad, randomize and every type but "hadamard" raise NotImplementedError naming
    the field.  `q_attn` / `k_cache` (on attention modules, with the scheme's `head_dim`) need a transformers PreTrainedModel — anything
    else raises upstream's ValueError (AttentionHookError) — and become a query hook on modeling.QuantizedAttentionImpl / a key hook on
    modeling.QuantizedKVCache that rotates the states over their last dimension, ahead of their quantization.
    `hadamard_weights`: a callable with the signature of upstream's `random_hadamard_matrix(size, dtype, device, gen)`
    (transform/utils/hadamard.py:53-77).  With it the `random-hadamard` type is accepted: every weight is drawn as
    RandomHadamardFactory draws it, factored (transform/random_hadamard.py) and applied by the kernels of csrc/ct_hadamard_k.hip;
    the table of known matrices behind that callable is upstream's and is not part of this package.  Without it the type
    raises as every other unsupported type does.
    `randomize=True` accepts schemes with `randomize=True`: the weight W[p][:, p] of transform/factory/hadamard.py:94-95, applied as
    a gather on each side of the rotation (csrc/ct_hadamard_perm.hip), never as a matrix.  The permutations are drawn as
    HadamardFactory draws them: one `torch.Generator()` per config group — seeded with `seed` when given, as
    TransformFactory.__init__ does; for `random-hadamard` the generator the weights are drawn from —, one CPU
    `torch.randperm(size)` per size at first use (after that size's weight), shared by every transform of the group with that
    size.  A scheme with `randomize=False` draws nothing.  Each transform keeps its permutation as the buffer `perm`."""
    ours = TransformConfig.coerce(config)
    for name, scheme in ours.config_groups.items():
        _check_supported(name, scheme, random_hadamard=hadamard_weights is not None, model=model, randomize=randomize)
    for name, scheme in ours.config_groups.items():
        random_weights = _RandomWeights(name, hadamard_weights, seed) if scheme.type == "random-hadamard" else None
        perms = None
        if scheme.randomize:
            generator = random_weights.generator if random_weights is not None else torch.Generator()
            if random_weights is None and seed is not None:
                generator.manual_seed(seed)
            perms = _Permutations(generator)
        for args in scheme.apply:
            for _, module in list(match_named_modules(model, args.targets, args.ignore)):
                _apply_to_module(name, scheme, module, args, random_weights, model, perms)
    setattr(model, TRANSFORM_CONFIG_NAME, config)
