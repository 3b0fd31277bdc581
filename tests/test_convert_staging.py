"""entrypoints/convert/staging.py without a GPU: the layout of a shard's outputs in one buffer (`output_layout`) and the copies that
bring it back (`d2h_chunks`), the two pure functions under the converters' round trip, and the names `converters` keeps exporting."""
import math
import os
import sys
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from compressed_tensors_amd.entrypoints.convert import converters, staging  # noqa: E402

Dtype = namedtuple("Dtype", "itemsize")  # all the layout reads of a dtype
B1, B2, B4 = Dtype(1), Dtype(2), Dtype(4)
READY = 4096  # the threshold, lowered from 32 MB so that small specs span several chunks

# names out of sorted order, sizes that are no multiples of 256, zero-element tensors first, last and in between
SPECS = [
    ("m.9.weight_scale", (33, 7), B2),        # 462 bytes
    ("m.1.weight_packed", (100, 30), B4),     # 12000 bytes: more than READY on its own
    ("m.5.weight", (0, 64), B2),              # zero elements, in the middle
    ("m.0.weight", (0,), B4),                 # zero elements, first in sorted order
    ("m.3.weight_zero_point", (3, 5), B4),    # 60 bytes
    ("m.2.weight_packed", (256,), B1),        # exactly one slot
    ("m.4.weight", (1000, 3), B1),            # 3000 bytes
    ("m.6.weight", (700,), B2),               # 1400 bytes
    ("m.7.weight", (1, 1), B1),               # 1 byte
    ("m.8.weight", (50, 50), B1),             # 2500 bytes
    ("m.9.weight_zero_point", (0, 0), B4),    # zero elements, last but one
    ("m.9.weight_shape", (2,), Dtype(8)),
]


def _check_layout(specs):
    slots, total = staging.output_layout(specs)
    assert list(slots) == sorted(name for name, _, _ in specs)
    end = 0
    for name in slots:
        off, n = slots[name]
        shape, dtype = next((s, d) for k, s, d in specs if k == name)
        assert n == math.prod(shape) * dtype.itemsize
        assert off % 256 == 0 and off >= end, name  # aligned, and past the end of every earlier slot
        end = max(end, off + n)
    last = list(slots)[-1] if slots else None
    assert total == (-(-sum(slots[last]) // 256) * 256 if last else 0)  # the end of the last slot
    assert total % 256 == 0 and total >= end
    return slots, total


def _check_chunks(slots, total, ready):
    chunks = staging.d2h_chunks(slots, total, ready)
    boundaries = {off for off, _ in slots.values()} | {total}
    at = 0
    for start, end, names in chunks:
        assert start == at and end >= start and end in boundaries and names
        at = end
    assert at == total  # [0, total) exactly once, in order
    assert all(end - start >= ready for start, end, _ in chunks[:-1])
    assert [name for _, _, names in chunks for name in names] == list(slots)  # every name once, in the writer's order
    for start, end, names in chunks:
        for name in names:
            off, n = slots[name]
            assert start <= off and off + n <= end, name  # a tensor's bytes arrive with the chunk its event follows
    return chunks


def test_layout_and_chunks_of_a_mixed_shard():
    slots, total = _check_layout(SPECS)
    assert total > 2 * READY
    assert slots["m.0.weight"] == (0, 0) and slots["m.1.weight_packed"] == (0, 12000) and slots["m.2.weight_packed"] == (12032, 256)
    assert slots["m.5.weight"][0] == slots["m.6.weight"][0]  # a zero-byte tensor takes no slot
    chunks = _check_chunks(slots, total, READY)
    assert len(chunks) >= 3
    assert chunks[0] == (0, 12032, ["m.0.weight", "m.1.weight_packed"])
    # the order of the specs does not matter
    assert staging.output_layout(sorted(SPECS)) == staging.output_layout(SPECS[::-1]) == (slots, total)


def test_layout_and_chunks_of_the_edge_shards():
    assert staging.output_layout([]) == ({}, 0) and staging.d2h_chunks({}, 0, READY) == []
    # nothing but zero-byte tensors: one empty chunk carries their names
    slots, total = _check_layout([("b", (0, 4), B2), ("a", (0,), B4)])
    assert total == 0 and _check_chunks(slots, total, READY) == [(0, 0, ["a", "b"])]
    # a single tensor, below and above the threshold
    for rows in (1, 5000):
        slots, total = _check_layout([("w", (rows, 3), B2)])
        assert _check_chunks(slots, total, READY) == [(0, total, ["w"])]
    # a zero-byte tensor behind a chunk that has just closed still belongs to a chunk
    slots, total = _check_layout([("a", (READY,), B1), ("b", (0,), B1)])
    assert _check_chunks(slots, total, READY) == [(0, READY, ["a"]), (READY, READY, ["b"])]


@pytest.mark.parametrize("ready", [1, 256, 1000, READY, 1 << 40])
def test_chunks_at_other_thresholds(ready):
    slots, total = _check_layout(SPECS)
    chunks = _check_chunks(slots, total, ready)
    if ready > total:
        assert len(chunks) == 1


def test_the_default_threshold_is_32_mb_and_the_names_stay_reachable_through_converters():
    assert staging._READY_BYTES == 32 << 20 and staging.d2h_chunks.__defaults__ == (staging._READY_BYTES,)
    for name in ("ReadyDict", "streaming_results", "_STREAMING", "_READY_BYTES", "_stage_to_device"):
        assert getattr(converters, name) is getattr(staging, name), name
    for name in ("match_name", "match_quantizable_tensors", "Converter", "build_inverse_weight_maps", "CompressedTensorsDequantizer",
                 "_ConfigDict"):
        assert hasattr(converters, name), name
