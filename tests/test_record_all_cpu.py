"""CPU: the public surface of `OpticalTable.record_all` (Monitor.record on every monitor of a table in one pass over the
segments) and the segment-source descriptor it hands to ot_monitor_record_many, built from a SegmentBatch as it lies in
memory — checked on CPU tensors, where the addresses are as good as on the device.  No library call is made."""
import os
import re

import torch

from optable_amd import abi
from optable_amd.batch import SegmentBatch
from optable_amd.engine import Engine, segment_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calls_exist():
    import optable_amd as oa

    assert callable(oa.OpticalTable.record_all)
    assert callable(Engine.monitor_record_many)


def test_binding_has_the_arguments_the_header_declares():
    text = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+ot_monitor_record_many\s*\(([^)]*)\)\s*;", text)
    assert decl, "ot_monitor_record_many is not declared in the header"
    restype, argtypes = abi.SYMBOLS["ot_monitor_record_many"]
    assert len(argtypes) == len(decl.group(1).split(",")) == 15
    assert abi.ABI_VERSION == 14  # an added function breaks no client


def _addresses(segs):
    return [segs.field(f).data_ptr() for f in abi.MON_FIELDS]


def test_source_of_a_tiled_fp32_batch_is_the_block_itself():
    n, K = 100, 3  # 300 slots -> 320, five tiles
    segs = SegmentBatch(n * K, "f32", "cpu", tiled=True)
    segs.count, segs.n_rays = torch.full((n,), K, dtype=torch.int32), n
    assert segs.layout == "tiled"
    src, n_segments, count, n_rays = segment_source(segs)
    tile = 64 * (12 * 4 + 8)
    block = segs.block.data_ptr()
    assert list(src.base) == [block + 64 * 4 * k for k in range(7)] == _addresses(segs)  # ox .. length are fields 0 .. 6 of a tile
    assert src.ray == block + 64 * 12 * 4
    assert (src.tile_stride, src.ray_stride, src.width, src.capacity) == (tile, tile, 4, 320)
    assert (n_segments, n_rays) == (300, n) and count is segs.count
    # the address rule on a slot in the fourth tile
    s = 3 * 64 + 17
    segs.dy.zero_()
    segs.dy[s // 64, s % 64] = 7.0
    at = src.base[4] + (s >> 6) * src.tile_stride + (s & 63) * src.width - block
    assert segs.block[at:at + 4].view(torch.float32).item() == 7.0


def test_source_of_planar_batches_in_slots_append_and_list_layouts():
    n, K = 70, 2
    slots = SegmentBatch(n * K, "f64", "cpu")
    slots.count, slots.n_rays = torch.full((n,), K, dtype=torch.int32), n
    src, n_segments, count, n_rays = segment_source(slots)
    assert list(src.base) == _addresses(slots) and src.ray == slots.ray.data_ptr()
    assert (src.tile_stride, src.ray_stride, src.width, src.capacity) == (512, 256, 8, n * K)
    assert (n_segments, n_rays) == (n * K, n) and count is slots.count

    app = SegmentBatch(200, "f32", "cpu", block=True)  # one allocation of 14 planes of 256 slots
    app.append, app.n_valid, app.count, app.n_rays = True, 130, torch.zeros(n, dtype=torch.int32), n
    src, n_segments, count, n_rays = segment_source(app)
    base = app.block.data_ptr()
    assert list(src.base) == [base + 256 * 4 * k for k in range(7)] and src.ray == base + 12 * 256 * 4
    assert (src.tile_stride, src.ray_stride, src.width, src.capacity) == (256, 256, 4, 256)
    assert (n_segments, count, n_rays) == (130, None, -1)  # a list with holes

    lst = SegmentBatch(50, "f64", "cpu")
    lst.n_valid = 33
    src, n_segments, count, n_rays = segment_source(lst)
    assert list(src.base) == _addresses(lst)
    assert (src.tile_stride, src.width) == (512, 8) and (n_segments, count, n_rays) == (33, None, 0)


def test_a_batch_of_no_rays_has_no_slots_to_scan():
    segs = SegmentBatch(0, "f64", "cpu")
    segs.count, segs.n_rays = torch.zeros(0, dtype=torch.int32), 0
    assert segment_source(segs)[1] == 0
