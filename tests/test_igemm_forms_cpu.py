"""The host-only plan queries of the fp32-MFMA conv kernels (mvg_conv_plan_query, mvg_conv_wgrad_tile): declared, bound, answering
without a GPU - they launch nothing; without a device the planners assume 256 CUs and one resident workgroup per CU - and
consistent, for every case of tests/test_igemm_forms_gpu.py, with the class table recomputed from the descriptor.  And the
enumerator of the stream-K unit space those tests name their structures with (igemm_forms_ref.streamk_structures), on unit
spaces written out by hand."""
import ctypes as C

import pytest

import cabi_header as hdr
import rot_mvgaze_amd  # noqa: F401
from rot_mvgaze_amd import _lib, ops
from rot_mvgaze_amd._lib import ConvDesc, ConvPlan

import igemm_forms_ref as ref
from igemm_forms_ref import BWD, FWD, streamk_structures



def desc(case):
    G, N, h, w_, cin, cout, k, st, pad = case
    return ConvDesc(G, N, h, w_, cin, cout, k, k, st, pad, (h + 2 * pad - k) // st + 1, (w_ + 2 * pad - k) // st + 1)


@pytest.fixture()
def reserve():
    """reserve(n): leave n CUs to the planners (0: all); reset afterwards."""
    cus = _lib.lib().mvg_device_cus()
    cus = cus if cus > 0 else 256
    try:
        yield lambda n: ops.set_reserved_cus(cus - n if n else 0)
    finally:
        ops.set_reserved_cus(0)


def test_plan_queries_are_declared_and_have_signatures():
    for name, nargs in (("mvg_conv_plan_query", 4), ("mvg_conv_wgrad_tile", 4)):
        assert name in hdr.functions, name + " is not declared in include/rotmvgaze.h"
        assert hdr.functions[name][0] == "int" and hdr.arity(name) == nargs
    # the plan struct: 15 int32 values (two arrays of 4 among them) and one int64, under these names
    assert C.sizeof(ConvPlan) == 15 * 4 + 4 + 8 and hdr.field_names("mvg_conv_plan") == \
        ["bm", "bn", "bk", "fasta", "ncls", "cls_tiles", "cls_kt", "streamk_grid", "splitk", "scratch_floats"]
    for k, name in enumerate(("MVG_PLAN_FPROP", "MVG_PLAN_FPROP_STATS", "MVG_PLAN_DGRAD", "MVG_PLAN_FUSER_FPROP")):
        assert hdr.constants[name] == k
    assert (_lib.PLAN_FPROP, _lib.PLAN_FPROP_STATS, _lib.PLAN_DGRAD, _lib.PLAN_FUSER_FPROP) == (0, 1, 2, 3)


def test_plan_queries_reject_bad_descriptors_and_tolerate_null():
    L = _lib.lib()
    bad = ConvDesc.make(1, 2, 8, 8, 48, 64, 3, 1, 1)            # 3x3 with 48 channels: not a power of two
    for kind in (_lib.PLAN_FPROP, _lib.PLAN_FPROP_STATS, _lib.PLAN_DGRAD):
        assert L.mvg_conv_plan_query(bad, kind, 0, None) == -1
    assert L.mvg_conv_wgrad_tile(bad, None, None, None) == -1
    with pytest.raises(RuntimeError, match="power-of-two"):
        ops.conv_plan_query(bad)
    with pytest.raises(RuntimeError, match="power-of-two"):
        ops.conv_wgrad_tile(bad)
    odd = ConvDesc.make(1, 2, 8, 8, 64, 6, 1, 1, 0)             # backward-data wants cout % 4 == 0, forward does not
    assert L.mvg_conv_plan_query(odd, _lib.PLAN_DGRAD, 0, None) == -1 and L.mvg_conv_plan_query(odd, _lib.PLAN_FPROP, 0, None) == 0
    ok = ConvDesc.make(1, 2, 8, 8, 64, 64, 1, 1, 0)
    assert L.mvg_conv_plan_query(None, 0, 0, None) == -1
    assert L.mvg_conv_plan_query(ok, 9, 0, None) == -1          # unknown kind
    assert L.mvg_conv_plan_query(ok, _lib.PLAN_FPROP, 0, None) == 0 and L.mvg_conv_wgrad_tile(ok, None, None, None) == 0


def test_plan_query_answers_without_a_device(reserve):
    """A one-tile conv is one 64x64 tile per workgroup; a Linear that cannot fill the device splits K into the caller's
    workspace and not without one; a stride-2 1x1 backward-data keeps only the parity class that has a tap."""
    pl = ops.conv_plan_query(desc((1, 1, 8, 8, 64, 64, 3, 1, 1)))
    assert pl == {"bm": 64, "bn": 64, "bk": 16, "fasta": True, "cls_tiles": [1], "cls_kt": [36], "streamk_grid": 0, "splitk": 1,
                  "scratch_floats": 0}
    lin = ConvDesc.linear(6, 512, 1536)
    assert ops.conv_plan_query(lin, _lib.PLAN_FPROP, 0)["splitk"] == 1
    with_ws = ops.conv_plan_query(lin, _lib.PLAN_FPROP, 16 * 6 * 1536)
    assert with_ws["splitk"] == 4 and with_ws["streamk_grid"] == 0        # 512 / 128: at least 128 k per split
    assert ops.conv_plan_query(lin, _lib.PLAN_FPROP_STATS, 16 * 6 * 1536)["splitk"] == 1
    pl = ops.conv_plan_query(desc((1, 2, 28, 28, 128, 256, 1, 2, 0)), _lib.PLAN_DGRAD)
    assert pl["cls_tiles"] == [(2 * 14 * 14 + pl["bm"] - 1) // pl["bm"] * (128 // pl["bn"])] and pl["cls_kt"] == [16]
    # with 8 CUs left a forward of 9 tiles x 144 K-steps is planned as stream-K whatever the occupancy, and asks for
    # two 128x128 slots per persistent workgroup
    reserve(8)
    pl = ops.conv_plan_query(desc((1, 5, 15, 15, 512, 128, 3, 1, 1)))
    assert (pl["bm"], pl["bn"], pl["bk"], pl["fasta"], pl["cls_tiles"], pl["cls_kt"]) == (128, 128, 32, True, [9], [144])
    assert pl["streamk_grid"] > 0 and pl["streamk_grid"] % 8 == 0 and pl["scratch_floats"] == pl["streamk_grid"] * 2 * 128 * 128
    assert pl["scratch_floats"] * 4 <= _lib.lib().mvg_scratch_bytes()


def test_wgrad_tile_query_matches_the_rule():
    """cout >= 128 and r*s*cin >= 128: 128x128; 64 <= cout: 64x128 / 64x64 / 128x32 by the columns; cout < 64: 32x128;
    incremental pixel addressing from ho * wo >= 32."""
    for case, form in ref.WGRAD_CASES + [(ref.WGRAD_SPLITS_CASE, (128, 128, True))]:
        d = desc(case)
        assert ops.conv_wgrad_tile(d) == form, case
        cols = d.r * d.s * d.cin
        want = (128, 128) if d.cout >= 128 and cols >= 128 else (64, 128) if d.cout >= 64 and cols >= 128 else \
            (64, 64) if d.cout >= 64 and cols >= 64 else (32, 128) if d.cout < 64 else (128, 32)
        assert form == want + (d.ho * d.wo >= 32,), case
    assert {f for _, f in ref.WGRAD_CASES} == {(bm, bn, incr) for bm, bn in ((128, 128), (64, 128), (64, 64), (32, 128), (128, 32))
                                               for incr in (True, False)}


def test_enumerator_on_hand_written_unit_spaces():
    # 4 tiles x 4 K-steps over 4 workgroups: every cut on a tile boundary, every tile whole
    assert streamk_structures([4], [4], 4) == set("af")
    # 3 tiles x 4 over 2 workgroups: cut at 6 = the middle of tile 1 (shared by two); both also hold a whole tile
    assert streamk_structures([3], [4], 2) == set("ab")
    # 1 tile x 9 over 3: shares [0,3) [3,6) [6,9) - the middle workgroup's whole share is a middle piece
    assert streamk_structures([1], [9], 3) == set("c")
    # 3 tiles x 4 over 4: cuts 3, 6, 9 - workgroups 1 and 2 hold a tail and a head (both slots), every tile has two owners
    assert streamk_structures([3], [4], 4) == set("bd")
    # 4 tiles x 4 over 2 workgroups of 8: cut on a boundary, whole tiles only
    assert streamk_structures([4], [4], 2) == set("af")
    # 5 tiles x 4 over 3: cuts 6, 13 - the middle workgroup [6,13) has the tail of tile 1, tile 2 whole and the head of tile 3
    assert streamk_structures([5], [4], 3) == set("abe")
    # two classes, 1 tile x 8 and 1 tile x 4, over 4 workgroups of 3: cuts 3, 6 inside class 0 and 9 inside class 1
    assert streamk_structures([1, 1], [8, 4], 4) == set("bcdgh")
    # ... over 3 workgroups of 4: cuts 4 and 8 - the second is the class boundary, no cut inside class 1
    assert streamk_structures([1, 1], [8, 4], 3) == set("abfh")
    # two classes of the same K length over 4 workgroups of 3: cuts 3 and 9 inside the classes, 6 between them: (g) without (h)
    assert streamk_structures([1, 1], [6, 6], 4) == set("bfg")
    # one workgroup: everything whole, nothing shared
    assert streamk_structures([2, 3], [5, 2], 1) == set("ah")
    # more workgroups than units: empty shares are skipped
    assert streamk_structures([1], [2], 4) == set("b")


def test_stream_k_cases_reach_every_structure_in_both_directions():
    """The (tiles, K-steps, persistent workgroups) of the stream-K cases - tiles and K-steps from the descriptor, the grid as the
    MI355X plans it (literal in the case table, asserted against the device by the GPU tests) - give the structures the table
    names, and between them (a)-(f) forward and (a)-(h) backward-data."""
    seen = {FWD: set(), BWD: set()}
    for direction, case, cus, (bm, bn, bk), grid, structures in ref.STREAMK_CASES:
        assert grid % cus == 0 and bm == 128 and bn >= 64
        tiles, kt = ref.class_counts(case, direction == BWD, bm, bn, bk)
        assert sum(t * k for t, k in zip(tiles, kt)) >= 8 * grid                 # >= 8 K-steps per workgroup: the planner's floor
        assert streamk_structures(tiles, kt, grid) == set(structures), (case, sorted(streamk_structures(tiles, kt, grid)))
        seen[direction] |= set(structures)
        k_max = max(taps * kc for _, taps, kc in ref.class_table(case, direction == BWD))
        assert k_max <= 4608, case                                                # the K the float64 bar is known to hold for
    assert seen[FWD] == set("abcdef") and seen[BWD] == set("abcdefgh")
    # stride 2 with a 3x3 and with a 7x7 filter: four classes of differing K
    assert ref.class_counts((1, 9, 11, 13, 128, 1024, 3, 2, 1), True, 128, 128, 16) == ([3, 3, 3, 3], [256, 128, 128, 64])
    assert ref.class_counts((1, 2, 17, 18, 64, 256, 7, 2, 3), True, 128, 64, 16) == ([2, 2, 2, 2], [256, 192, 192, 144])
    # 9x9 at stride 2: parity classes of 25 / 20 / 20 / 16 pixels with 1 / 2 / 2 / 4 taps, run longest K first
    assert ref.class_table((1, 1, 9, 9, 64, 1024, 3, 2, 1), True) == [(16, 4, 1024), (20, 2, 1024), (20, 2, 1024), (25, 1, 1024)]


def test_query_classes_equal_the_counts_recomputed_from_the_descriptor(reserve):
    """For every descriptor of the GPU file, under the CU counts it runs with and with every CU: cls_tiles and cls_kt of the
    query are the class table of the descriptor cut into the tile the query reports (host arithmetic; the tile itself may
    differ from the device's, whose occupancies this machine does not know)."""
    runs = [(dr, case, cus) for dr, case, cus, _, _, _ in ref.STREAMK_CASES] + [(dr, case, ref.PLAIN_CUS) for dr, case, _ in ref.PLAIN_CASES]
    runs += [(dr, case, 0) for dr, case, _ in runs]
    import test_kernels_gpu
    runs += [(dr, case, 0) for case in test_kernels_gpu.CONV_CASES for dr in (FWD, BWD)]
    for direction, case, cus in runs:
        reserve(cus)
        for kind in ((_lib.PLAN_DGRAD,) if direction == BWD else (_lib.PLAN_FPROP, _lib.PLAN_FPROP_STATS)):
            pl = ops.conv_plan_query(desc(case), kind)
            assert (pl["bm"], pl["bn"]) in ((128, 128), (128, 64), (64, 64), (128, 32))
            assert pl["bk"] == (32 if (pl["bm"], pl["bn"], direction) == (128, 128, FWD) else 16)
            tiles, kt = ref.class_counts(case, direction == BWD, pl["bm"], pl["bn"], pl["bk"])
            assert (pl["cls_tiles"], pl["cls_kt"]) == (tiles, kt), (direction, case, cus, pl)
            k_per_tap = case[5] if direction == BWD else case[4]
            taps = max(t for _, t, _ in ref.class_table(case, direction == BWD))          # the uniform-tap loader masks <= 32 taps
            assert pl["fasta"] == (pl["bn"] > 32 and k_per_tap % pl["bk"] == 0 and taps <= 32), (direction, case, pl)
            assert pl["scratch_floats"] == pl["streamk_grid"] * 2 * pl["bm"] * pl["bn"] and pl["splitk"] == 1
            assert pl["streamk_grid"] == 0 or (pl["bm"] == 128 and pl["bn"] >= 64 and sum(t * k for t, k in zip(tiles, kt)) >= 8 * pl["streamk_grid"])
    # the plain cases are plain, and run the instantiation they are listed for, whatever the occupancy
    reserve(ref.PLAIN_CUS)
    for direction, case, form in ref.PLAIN_CASES:
        pl = ops.conv_plan_query(desc(case), _lib.PLAN_DGRAD if direction == BWD else _lib.PLAN_FPROP)
        assert (pl["bm"], pl["bn"], pl["bk"], pl["fasta"], pl["streamk_grid"]) == form + (0,), (case, pl)
