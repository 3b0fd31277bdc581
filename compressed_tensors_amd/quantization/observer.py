"""A min-max calibration observer on the device: the call surface of the reference tests' observer
(`Observer(base_name, args, module)`, `forward(observed) -> (scale, zero_point)`, `.min_vals` / `.max_vals` after a call) over the
strided launch of csrc/ct_attn_observe.hip.

It serves the states the static QDQ of csrc/ct_attn.hip consumes — `q` / `k` / `v` under the `tensor` and `attn_head`
strategies, read in place through the strides an attention module passes — and `input` / `output` activations under `tensor`
(the static W8A8 case: the tensor strategy reduces everything, so a `(..., hidden)` activation is one scale entry whose rows are
`hidden` long), and the calibrated half of the NVFP4 preset's `tensor_group`, `dynamic="local"` activations: `get_global_scale`, the float32
global scale under which forward_quantize computes the local scales per call.  Weights stay with `calculate_qparams_from_weight`, which fuses their observer with the scale computation.

No arithmetic lives here: the running extremes are 32-bit order keys in a caller-visible buffer (`state`), folded and turned into
scale / zero point by the kernel."""
import weakref
from typing import Optional, Tuple

import torch

from .. import codec
from .quant_args import enum_value

__all__ = ["MinMaxObserver", "OBSERVERS", "observe_key_value"]

# observer name -> keep: "memoryless_minmax" — each call stands alone; "static_minmax" — the extremes of every call since reset()
OBSERVERS = {"memoryless_minmax": False, "static_minmax": True}
_ATTENTION, _ACTIVATION = ("q", "k", "v"), ("input", "output")


class MinMaxObserver(torch.nn.Module):
    """`observer`: "memoryless_minmax" or "static_minmax" (None: `args.observer`, and where the arguments name none, the
    reference's default for static arguments, "memoryless_minmax").  "minmax" (the moving average) and anything else:
    NotImplementedError.  With `scale` / `zero_point` (module parameters of the reference's shapes), the kernel writes them in
    place and forward returns them."""

    def __init__(self, base_name: str, args, module: Optional[torch.nn.Module] = None, observer: Optional[str] = None):
        super().__init__()
        name = observer if observer is not None else (getattr(args, "observer", None) or "memoryless_minmax")
        if name not in OBSERVERS:
            raise NotImplementedError(f"observer {name!r} is not implemented by the MI355X path ({', '.join(sorted(OBSERVERS))} are)")
        strategy = enum_value(args.strategy)
        if base_name == "weight":
            raise NotImplementedError("weights are observed by calculate_qparams_from_weight (quantization/utils.py), which fuses the observer "
                                      "with the scale computation; MinMaxObserver serves q / k / v and input / output")
        dynamic = enum_value(getattr(args, "dynamic", False))
        # the NVFP4 preset's activations (tensor_group, dynamic="local"): the local scales are forward_quantize's, per call; the GLOBAL scale is
        # calibrated — get_global_scale below
        self.global_only = base_name in _ACTIVATION and strategy == "tensor_group" and dynamic == "local"
        if base_name in _ACTIVATION:
            if strategy != "tensor" and not self.global_only:
                raise NotImplementedError(f"a static {strategy!r} observer of {base_name} activations is not implemented by the MI355X path (tensor is, and "
                                          "tensor_group with dynamic='local' for its global scale)")
        elif base_name not in _ATTENTION:
            raise ValueError(f"Unknown quantization base name: {base_name}")
        if dynamic in (True, "local") and not self.global_only:
            raise NotImplementedError("dynamic arguments are not observed: forward_quantize computes their scales per call")
        self.parent = weakref.ref(module) if module is not None else (lambda: None)
        self.base_name = base_name
        self.args = args
        self.observer = name
        self.keep = OBSERVERS[name]
        self.min_vals = None
        self.max_vals = None
        self._state = None
        self._global_state = None

    def _kwargs(self):
        a = self.args
        return dict(num_bits=int(a.num_bits), symmetric=bool(a.symmetric), qtype=enum_value(getattr(a, "type", "int")), strategy=enum_value(a.strategy),
                    zp_dtype=getattr(a, "zp_dtype", None), keep=self.keep, want_minmax=True)

    def state_for(self, observed: torch.Tensor) -> torch.Tensor:
        """the running state, armed on first use (and again when the entry count or the device changes)"""
        entries = codec.plan_attn_observe(observed.shape, observed.stride(), observed.dtype, self.args.strategy).entries  # shapes only; the call checks the device
        if self._state is None or self._state.shape[1] != entries or self._state.device != observed.device:
            self._state = codec.attn_observe_state(entries, observed.device)
        return self._state

    def reset(self) -> None:
        """forget every call so far: the state is armed again (in place; nothing waits)"""
        for state in (self._state, self._global_state):
            if state is not None:
                codec.attn_observe_arm(state)
        self.min_vals = self.max_vals = None

    def _global_scale(self):
        parent = self.parent()
        return getattr(parent, f"{self.base_name}_global_scale", None) if parent is not None else None

    def get_global_scale(self, observed: torch.Tensor, global_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the reference observer's get_global_scale: generate_gparam of the extremes of the WHOLE tensor (its `reshape((1, 1, -1))`, read in
        place through the strides), float32 (1,) — of this call alone ("memoryless_minmax") or of every call since reset() ("static_minmax").
        `global_scale` (a module's `{base_name}_global_scale` parameter): the kernel writes it in place and it is what is returned."""
        if self._global_state is None or self._global_state.device != observed.device:
            self._global_state = codec.attn_observe_state(1, observed.device)
        return codec.attn_observe_global_scale(observed, self._global_state, keep=self.keep, global_scale=global_scale)

    def forward(self, observed: torch.Tensor, scale: Optional[torch.Tensor] = None, zero_point: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.global_only:
            raise NotImplementedError("dynamic arguments are not observed: forward_quantize computes their local scales per call (get_global_scale "
                                      "calibrates the global one)")
        scale, zero_point, self.min_vals, self.max_vals = codec.attn_observe(
            observed, self.state_for(observed), scale=scale, zero_point=zero_point, global_scale=self._global_scale(), **self._kwargs())
        return scale, zero_point


def observe_key_value(k_observer: MinMaxObserver, v_observer: MinMaxObserver, key: torch.Tensor, value: torch.Tensor, *, k_scale=None, v_scale=None,
                      k_zero_point=None, v_zero_point=None):
    """the forward of both observers on the K and V of one cache update through ONE ct_attn_observe (codec.attn_observe_pair): the
    arguments are `k_observer`'s, which the two share; each keeps its own state and `min_vals` / `max_vals`.  Returns
    ((k_scale, k_zero_point), (v_scale, v_zero_point))."""
    k_out, v_out = codec.attn_observe_pair(
        key, value, k_observer.state_for(key), v_observer.state_for(value), k_scale=k_scale, v_scale=v_scale, k_zero_point=k_zero_point,
        v_zero_point=v_zero_point, **k_observer._kwargs())
    k_scale, k_zero_point, k_observer.min_vals, k_observer.max_vals = k_out
    v_scale, v_zero_point, v_observer.min_vals, v_observer.max_vals = v_out
    return (k_scale, k_zero_point), (v_scale, v_zero_point)
