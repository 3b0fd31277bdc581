"""The host side of one shard's round trip, shared by the converters: the shard's tensors go to the GPU through one pinned buffer
and one copy (`_stage_to_device`), every output lives in ONE device buffer (`device_outputs`), one launch per table the library's
planner accepts converts them (`launch_tables`; `table_calls` gives its plan and launch for a table of `codec._TABLES`), and the
results come back through one pinned buffer with an event behind every ~32 MB (`return_to_host`); `settle` synchronises unless the caller streams its results.  `output_layout` and `d2h_chunks` are
pure functions of the output specs `[(name, shape, dtype)]`."""
import array
import contextlib
import ctypes
import math
import threading

import torch

_ALIGN = 256  # every tensor starts on a 256-byte boundary of a staging / output buffer
_READY_BYTES = 32 << 20  # one event per ~32 MB of D2H copies


_STREAMING = threading.local()


@contextlib.contextmanager
def streaming_results():
    """inside this context (per thread) a converter that supports it hands its tensors over while their D2H copies are still in flight"""
    prev = getattr(_STREAMING, "on", False)
    _STREAMING.on = True
    try:
        yield
    finally:
        _STREAMING.on = prev


class ReadyDict(dict):
    """a shard's converted tensors: host tensors whose device-to-host copies may still be in flight.  `ready[name]` is the event
    recorded behind the copy of `name` (absent: the tensor is complete); `keep` holds what must stay alive until then.  Consumers
    that do not know about it call `wait()` first."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ready = {}
        self.keep = []

    def wait(self, name=None) -> None:
        if name is not None:
            ev = self.ready.pop(name, None)
            if ev is not None:
                ev.synchronize()
            return
        for ev in set(self.ready.values()):
            ev.synchronize()
        self.ready.clear()
        self.keep.clear()


def _stage_to_device(state_dicts, dev, host_only=()):
    """Move a shard's compressed tensors to the device through ONE pinned buffer and ONE copy.  The tensors safetensors
    hands out are lazily mapped file pages: `t.to(device)` per tensor is a pageable copy that faults the file in 4 KB at a
    time on the calling thread (23.0 ms for the 125 MB of a TinyLlama-shaped shard, half of `process`).  Here the I/O
    threads copy the mapped pages into the pinned buffer in parallel, one asynchronous H2D moves it (6.7 ms together), and
    the device tensors are views into the device buffer (256-byte aligned).  Replaces the entries of `state_dicts` in place; returns what must stay alive until
    the stream is synchronised."""
    from .safetensors_io import host_bytes, parallel_copy

    plan, off = [], 0
    for sd in state_dicts:
        for key, t in sd.items():
            if key in host_only or t is None or t.device.type != "cpu":
                continue
            t = t.contiguous()
            n = t.numel() * t.element_size()
            plan.append((sd, key, t, off, n))
            off += (n + _ALIGN - 1) // _ALIGN * _ALIGN
    if not plan:
        return None
    stage = torch.empty(off, dtype=torch.uint8, pin_memory=True)
    flat = stage.numpy()
    parallel_copy([(flat[o:o + n], host_bytes(t)) for _, _, t, o, n in plan if n])
    dbuf = stage.to(dev, non_blocking=True)
    for sd, key, t, o, n in plan:
        sd[key] = dbuf[o:o + n].view(t.dtype).view(t.shape)
    return stage, dbuf


def stage_inputs(out, inputs, dev) -> None:
    """the host tensors of `inputs` (one dict per module) become views of one staged device buffer, kept alive by `out.keep`"""
    out.keep.append(_stage_to_device(inputs, dev))
    for sd in inputs:  # tensors handed over on the device already are not staged
        for k in sd:
            sd[k] = sd[k].contiguous()


def output_layout(specs):
    """({name: (offset, nbytes)}, total bytes) of the outputs `[(name, shape, dtype)]` in one buffer: in the order the writer stores
    the tensors (sorted names), each in a slot of whole 256-byte units (a zero-byte tensor takes none)"""
    slots, off = {}, 0
    for name, shape, dtype in sorted(specs, key=lambda spec: spec[0]):
        n = math.prod(shape) * dtype.itemsize
        slots[name] = (off, n)
        off += -(-n // _ALIGN) * _ALIGN
    return slots, off


def d2h_chunks(slots, total, ready_bytes=_READY_BYTES):
    """[(start, end, names)]: the copies that bring a buffer laid out by `output_layout` back, each ending on a tensor boundary and
    closed once it spans `ready_bytes` or the tensors run out.  Every name belongs to exactly one chunk."""
    order = list(slots)
    chunks, start, pending = [], 0, []
    for i, name in enumerate(order):
        pending.append(name)
        end = slots[order[i + 1]][0] if i + 1 < len(order) else total
        if end - start >= ready_bytes or i + 1 == len(order):
            chunks.append((start, end, pending))
            start, pending = end, []
    return chunks


def _views(buf, specs, slots):
    views = {}
    for name, shape, dtype in specs:
        off, n = slots[name]
        views[name] = buf[off:off + n].view(dtype).view(shape)
    return views


def device_outputs(specs, dev):
    """(buffer, {name: view}): every output of the shard in ONE uint8 device buffer"""
    slots, total = output_layout(specs)
    dbuf = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    return dbuf, _views(dbuf, specs, slots)


def plan_tables(items, modules, item_type, plan):
    """[(n, table, workgroups)]: the ctypes `items` in as few tables as the library's `plan` accepts (a refused batch is halved; a
    refused single item is malformed and raises, naming its module)"""
    from ... import _lib

    if not items:
        return []
    table = (item_type * len(items))(*items)
    blocks = int(plan(ctypes.cast(table, ctypes.c_void_p), len(items)))
    if blocks >= 0:
        return [(len(items), table, blocks)]
    if len(items) == 1:
        raise ValueError(f"{modules[0]}: {_lib.last_error()}")
    half = len(items) // 2
    return plan_tables(items[:half], modules[:half], item_type, plan) + plan_tables(items[half:], modules[half:], item_type, plan)


def table_calls(kind: str, d: int, scalars):
    """the `plan` and `launch` of `launch_tables` for a table of `codec._TABLES`, from the (kind, d, scalars) that codec's `rtn_*_launch` functions
    give: the symbols are resolved through the registry, so a converter names no library function and rebuilds no argument list"""
    from ... import _lib
    from ...codec import _TABLES

    plan_symbol, directed, launch_symbol = _TABLES[kind]
    lib = _lib.load()
    plan_fn = getattr(lib, plan_symbol)
    launch_fn = getattr(lib, launch_symbol if isinstance(launch_symbol, str) else launch_symbol[d])
    plan = (lambda table, n: plan_fn(table, n, d)) if directed else plan_fn
    return plan, lambda table, n, blocks, handle: launch_fn(table, n, blocks, *scalars, handle)


def launch_tables(items, modules, item_type, plan, launch, dev) -> None:
    """upload every table of `plan_tables` and hand it to `launch(table_ptr, n, workgroups, stream_handle)` on `dev`'s current stream"""
    from ... import _lib
    from ...codec import _upload_table

    stream = torch.cuda.current_stream(dev)
    for n, table, blocks in plan_tables(items, modules, item_type, plan):
        dtable = _upload_table(array.array("q", bytes(table)), dev)
        _lib.check(launch(dtable.data_ptr(), n, blocks, _lib.stream_on(dev)))
        dtable.record_stream(stream)


def return_to_host(out: ReadyDict, specs, dbuf, stream) -> None:
    """`out[name]` = the host tensor of every output of `device_outputs`, `out.ready[name]` = the event behind its copy.  Back
    through one pinned buffer, in copies of ~32 MB that end on tensor boundaries, an event behind each: the writer waits for a
    tensor's event, not for the whole shard"""
    slots, total = output_layout(specs)
    stage = torch.empty(dbuf.numel(), dtype=torch.uint8, pin_memory=True)
    host = _views(stage, specs, slots)
    for start, end, names in d2h_chunks(slots, total):
        if end > start:
            stage[start:end].copy_(dbuf[start:end], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        for name in names:
            out[name] = host[name]
            out.ready[name] = ev
    out.keep.append(dbuf)


def settle(out: ReadyDict, stream, stream_results: bool) -> None:
    """unless the converter streams its results (`stream_results`, or inside `streaming_results()`): wait for the copies and let
    go of the staging buffers"""
    if not (stream_results or getattr(_STREAMING, "on", False)):
        stream.synchronize()
        out.ready.clear()
        out.keep.clear()  # the list lives on in the returned ReadyDict: empty it, or the pinned staging stays alive for the shard's lifetime
