"""The ABI of the overlap queries (include/voxels_hip.h, "overlap queries"): the two exports, the binding's names, and the layout
of the four records as the C compiler sees them."""
import os
import re

import overlap_oracle as oo
import voxels_amd
from voxels_amd import binding


def test_the_library_exports_vx_overlap_boxes():
    lib = binding.HipLibrary()
    assert lib.has_overlap and hasattr(lib.lib, "vx_overlap_boxes") and hasattr(lib.lib, "vx_overlap_boxes_device")
    for name in ("overlap_boxes", "overlap_boxes_raw", "overlap_boxes_device"):
        assert hasattr(binding.Polygonizer, name)
    for name in ("OVERLAP_BOX_DTYPE", "OVERLAP_TRI_DTYPE", "OVERLAP_RANGE_DTYPE", "OVERLAP_COUNTS_DTYPE", "OVERLAP_MAX_QUERIES", "overlap_boxes"):
        assert name in voxels_amd.__all__ and getattr(voxels_amd, name) is getattr(binding, name)


def test_record_layout():
    # as the C compiler lays out the header's structs (tests/overlap/overlap_host.cpp includes include/voxels_hip.h)
    layout = [oo.load().ov_layout(k) for k in range(24)]
    assert layout[:6] == [32, 16, 8, 32, 48, 156] and layout[22] == binding.OVERLAP_MAX_QUERIES == 1 << 20 and layout[23] == 0xFFFFFFFF
    B, T, R, K = binding.OVERLAP_BOX_DTYPE, binding.OVERLAP_TRI_DTYPE, binding.OVERLAP_RANGE_DTYPE, binding.OVERLAP_COUNTS_DTYPE
    assert [B.itemsize, T.itemsize, R.itemsize, K.itemsize] == layout[:4]
    assert binding.VERTEX_DTYPE.itemsize == 48 and binding.LISTED_BLOCK_DTYPE.itemsize == 156
    assert B.names == ("lo", "reserved0", "hi", "reserved1") and T.names == ("query", "entry", "block_id", "tri")
    assert R.names == ("first", "count") and K.names == ("triangles", "pairs", "queries", "hit_queries", "max_per_query", "reserved")
    offsets = [d.fields[k][1] for d in (B, T, R, K) for k in d.names]
    assert offsets == layout[6:22] == [0, 12, 16, 28, 0, 4, 8, 12, 0, 4, 0, 8, 16, 20, 24, 28]


def test_the_box_helper():
    b = binding.overlap_boxes([[0, 1, 2], [3, 4, 5]], [[6, 7, 8], [9, 10, float("inf")]])
    assert b.dtype == binding.OVERLAP_BOX_DTYPE and b["lo"].tolist() == [[0, 1, 2], [3, 4, 5]] and b["hi"][1].tolist() == [9, 10, float("inf")]
    assert not b["reserved0"].any() and not b["reserved1"].any()
    assert len(binding.overlap_boxes([0, 0, 0], [1, 1, 1])) == 1


def test_the_header_states_the_limit_and_the_prototypes():
    text = open(os.path.join(oo.ROOT, "include", "voxels_hip.h")).read()
    assert re.search(r"#define VX_OVERLAP_MAX_QUERIES \(1u << 20\)", text)
    flat = re.sub(r"\s+", " ", text)
    assert ("int vx_overlap_boxes_device(vx_ctx*, uint32_t level, const vx_overlap_box* d_boxes, uint32_t n, uint32_t capacity, "
            "vx_overlap_tri* d_tris, float* d_corners /* may be NULL */, vx_overlap_range* d_ranges /* may be NULL */, "
            "vx_overlap_counts* d_counts);") in flat
    assert ("int vx_overlap_boxes(vx_ctx*, uint32_t level, const vx_overlap_box* boxes, uint32_t n, uint32_t capacity, "
            "vx_overlap_tri* tris, float* corners, vx_overlap_range* ranges, vx_overlap_counts* counts);") in flat
    assert "A separating-axis refinement is out of scope" in text and "by the block's coord_id ascending" in text
