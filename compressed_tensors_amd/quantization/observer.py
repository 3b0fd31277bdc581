"""A min-max calibration observer on the device: the call surface of the reference tests' observer
(`Observer(base_name, args, module)`, `forward(observed) -> (scale, zero_point)`, `.min_vals` / `.max_vals` after a call) over the
strided launch of csrc/ct_attn_observe.hip.

It serves the states the static QDQ of csrc/ct_attn.hip consumes — `q` / `k` / `v` under the `tensor` and `attn_head`
strategies, read in place through the strides an attention module passes — and `input` / `output` activations under `tensor`
(the static W8A8 case: the tensor strategy reduces everything, so a `(..., hidden)` activation is one scale entry whose rows are
`hidden` long).  Weights stay with `calculate_qparams_from_weight`, which fuses their observer with the scale computation.

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
        if base_name in _ACTIVATION:
            if strategy != "tensor":
                raise NotImplementedError(f"a static {strategy!r} observer of {base_name} activations is not implemented by the MI355X path (tensor is)")
        elif base_name not in _ATTENTION:
            raise ValueError(f"Unknown quantization base name: {base_name}")
        if enum_value(getattr(args, "dynamic", False)) in (True, "local"):
            raise NotImplementedError("dynamic arguments are not observed: forward_quantize computes their scales per call")
        self.parent = weakref.ref(module) if module is not None else (lambda: None)
        self.base_name = base_name
        self.args = args
        self.observer = name
        self.keep = OBSERVERS[name]
        self.min_vals = None
        self.max_vals = None
        self._state = None

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
        if self._state is not None:
            codec.attn_observe_arm(self._state)
        self.min_vals = self.max_vals = None

    def _global_scale(self):
        parent = self.parent()
        return getattr(parent, f"{self.base_name}_global_scale", None) if parent is not None else None

    def forward(self, observed: torch.Tensor, scale: Optional[torch.Tensor] = None, zero_point: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
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
