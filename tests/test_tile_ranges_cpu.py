"""tests/tile_ranges_ref.py (the model of the persistent kernels' tile ranges) against the sources it copies, and what it says about the
shapes of the two convolution route suites: the tile-edge shapes reach no hand-over class, the many-tile shapes reach every one."""
import os
import re

import pytest

import test_gpu_conv2d_routes as G2
import test_gpu_conv3d_routes as G3
import tile_ranges_ref as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "estdepth_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(pattern, text, name, what):
    m = re.search(pattern, text)
    assert m, "%s: no %s (%s)" % (name, what, pattern)
    return int(m.group(1))


# ------------------------------------------------------------------------------------------------------------- model vs sources
def test_grid_formula_is_the_one_of_estd_common_h():
    text = _src("estd_common.h")
    body = text[text.index("static inline int estd_persistent_wgs"):text.index("estd_conv3d_volume_fits_rsrc")]
    for piece in ("estd_device_cus() - estd_get_reserved_cus()", "(cus > 8 ? cus : 8) * per_cu", "total < slots ? (int)total : slots",
                  "if (grid >= 8) grid &= ~7;"):
        assert piece in body, "estd_common.h: %s" % piece
    clamp = _src("est_fusion.hip")
    assert "n > 128 ? 128 : n; return (n + 7) & ~7;" in clamp, "est_fusion.hip: the reserve's clamp (0 .. 128, multiples of 8)"
    assert max(T.RESERVES) == 128
    # (total, cus, reserved, per_cu) -> grid, by hand
    for args, want in (((66, 256, 0, 1), 64), ((4800, 256, 0, 1), 256), ((2400, 256, 0, 2), 512), ((2400, 256, 128, 2), 256),
                       ((7, 256, 0, 1), 7), ((1440, 256, 128, 1), 128), ((100, 8, 8, 2), 16), ((120, 256, 0, 2), 120), ((90, 256, 0, 2), 88)):
        assert T.grid(*args) == want, args


@pytest.mark.parametrize("src", sorted({f["src"] for f in list(T.CONV3D.values()) + list(T.CONV2D.values())}))
def test_range_formula_is_the_one_of_the_kernel(src):
    text = _src(src)
    n = len(re.findall(r"const int r = \(\(G & 7\) == 0\) \? \(bid & 7\) \* \(G >> 3\) \+ \(bid >> 3\) : bid;", text))
    kernels = 2 if src == "conv2d_wino2.hip" else 1              # (its two item widths are two functions)
    assert n == kernels, "%s: the XCD mapping of blockIdx" % src
    assert len(re.findall(r"u0? = \(int\)\(\(long long\)total_\w+ \* r / G\);", text)) == kernels, "%s: u" % src
    assert len(re.findall(r"u_end = \(int\)\(\(long long\)total_\w+ \* \(r \+ 1\) / G\);", text)) == kernels, "%s: u_end" % src


@pytest.mark.parametrize("family", sorted(T.CONV3D))
def test_conv3d_table_agrees_with_its_launcher(family):
    f = T.CONV3D[family]
    text = _src(f["src"])
    assert _int(r"constexpr int [^;]*?\bTH = (\d+)", text, f["src"], "TH") == f["th"], f["src"]
    assert _int(r"constexpr int [^;]*?\bTW = (\d+)", text, f["src"], "TW") == f["tw"], f["src"]
    assert _int(r"estd_persistent_grid\(\s*\w+\s*,\s*(\d+)\s*\)", text, f["src"], "per_cu") == f["per_cu"], f["src"]
    assert len(re.findall(r"estd_persistent_grid\(", text)) == 1, f["src"]
    total = re.search(r"const (?:int|long long) total = ([^;]+);", text)
    assert total, "%s: total" % f["src"]
    if f["depth"] == "pairs":
        assert "dpairs = (d.D + 1) / 2" in text and total.group(1) == "(long long)d.N * dpairs * tiles_h * tiles_w", (f["src"], total.group(1))
        assert "seg_end = min(u_end, (col + 1) * dpairs)" in text and "col = u / dpairs" in text, f["src"]
    else:
        assert total.group(1) == "d.N * d.D * tiles_h * tiles_w", (f["src"], total.group(1))
        assert "seg_end = min(u_end, (col + 1) * D)" in text and "col = u / D" in text, f["src"]
    assert "twi = col % tiles_w, c2 = col / tiles_w" in text and "thi = c2 % tiles_h, n = c2 / tiles_h" in text, "%s: the column decode" % f["src"]


@pytest.mark.parametrize("family", sorted(T.CONV2D))
def test_conv2d_table_agrees_with_its_launcher(family):
    f = T.CONV2D[family]
    text = _src(f["src"])
    th, tw = (_int(r"constexpr int [^;]*?\b%s = (\d+)" % k, text, f["src"], k) for k in ("TH", "TW"))
    assert tw == f["tw"], f["src"]
    assert _int(r"estd_persistent_grid\(\s*\w+\s*,\s*(\d+)\s*\)", text, f["src"], "per_cu") == f["per_cu"], f["src"]
    if family.startswith("wino2"):
        assert _int(r"#define ESTD_C2W2_SPLIT (\d)", text, f["src"], "ESTD_C2W2_SPLIT") == 1, f["src"]
        for piece in ("wide = ESTD_C2W2_SPLIT != 0 && (d.cout & 63) == 0;", "const int th = wide ? TH / 2 : TH;",
                      "tiles_h = (d.H + th - 1) / th;", "groups = d.cout / (wide ? 64 : 32);", "total = (long long)groups * d.N * tiles_h * tiles_w;"):
            assert piece in text, "%s: %s" % (f["src"], piece)
        assert (f["th"], f["group"]) == ((th // 2, 64) if family == "wino2_wide" else (th, 32)), f["src"]
    else:
        for piece in ("tiles_h = (d.H + TH - 1) / TH;", "groups = d.cout / (16 * NT);", "total = groups * d.N * tiles_h * tiles_w;"):
            assert piece in text, "%s: %s" % (f["src"], piece)
        assert (f["th"], f["group"]) == (th, 16 * int(family[-1])), f["src"]
    n_decode = 2 if f["src"] == "conv2d_wino2.hip" else 1
    for piece in ("tiles_per_group = p.N * tiles_h * tiles_w;", "grp = item / tiles_per_group;", "int t = item - grp * tiles_per_group;",
                  "const int twi = t % tiles_w; t /= tiles_w;", "const int thi = t % tiles_h; n = t / tiles_h;"):
        assert text.count(piece) == n_decode, "%s: the item decode (%s)" % (f["src"], piece)


def test_model_is_consistent_with_itself():
    for total, G in ((1440, 256), (1176, 128), (7, 7), (66, 64), (2400, 512)):
        rs = T.ranges(total, G)
        assert rs[0][0] == 0 and rs[-1][1] == total and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
        assert sorted(T.range_of_block(b, G) for b in range(G)) == list(range(G))
    for family in T.CONV3D:
        for dims in T.ranges3d(family) + G3.SMALL:
            tiles_h, tiles_w, col, total = T.geometry3d(family, dims)
            order = [(n, thi, twi, dp) for n in range(dims[0]) for thi in range(tiles_h) for twi in range(tiles_w) for dp in range(col)]
            assert [T.decode3d(family, dims, u) for u in range(total)] == order
            c = T.classes3d(family, dims)
            assert c["only"] + c["first"] + c["middle"] + c["last"] == total and c["first"] == c["last"]
    for family, cout in (("wino2", 96), ("wino2_wide", 320), ("k3_nt2", 96), ("k3_nt4", 192)):
        shape = (5, 9, 17)
        groups, tiles_h, tiles_w, total = T.geometry2d(family, shape, cout)
        order = [(g, n, thi, twi) for g in range(groups) for n in range(shape[0]) for thi in range(tiles_h) for twi in range(tiles_w)]
        assert [T.decode2d(family, shape, cout, i) for i in range(total)] == order
        c = T.classes2d(family, shape, cout)
        assert c["same_image"] + c["next_image"] + c["next_group"] == total - c["G"]


def test_model_reproduces_the_hand_counts_of_the_starting_shapes():
    """(120, 5, 9, 17) and (14, 41, 9, 17) at 256 CUs, counted independently of the model when the shapes were proposed"""
    c = T.classes3d("wino3", (120, 5, 9, 17))
    assert (c["G"], c["len_min"], c["len_max"], c["middle"], c["whole_inside"], c["cross_n"], c["odd_last_start"]) == (256, 5, 6, 320, 128, 96, 64)
    c = T.classes3d("direct", (120, 5, 9, 17))
    assert (c["G"], c["len_min"], c["len_max"]) == (512, 4, 5)
    c = T.classes3d("direct", (120, 5, 9, 17), reserved=128)
    assert (c["G"], c["whole_inside"]) == (256, 160)
    c, c128 = T.classes3d("wino2", (14, 41, 9, 17)), T.classes3d("wino2", (14, 41, 9, 17), reserved=128)
    assert (c["len_min"], c["len_max"], c["middle"], c128["len_min"], c128["len_max"], c128["middle"]) == (4, 5, 608, 9, 10, 832)
    # the model's launches of the full-size volumes: 4800 tiles in ranges of 18-19, 14400 in ranges of 56-57 with 186 whole columns
    c = T.classes3d("wino3", (1, 64, 120, 160))
    assert (c["total"], c["G"], c["len_min"], c["len_max"], c["whole_inside"], c["cross_n"]) == (4800, 256, 18, 19, 0, 0)
    c = T.classes3d("wino3", (3, 64, 120, 160))
    assert (c["total"], c["len_min"], c["len_max"], c["whole_inside"], c["cross_n"]) == (14400, 56, 57, 186, 2)


# --------------------------------------------------------------------------------------------------- the shapes of the two suites
def _small_cases():
    return [p.values[0] for p in G3.CASES if p.values[0]["shapes"] is G3.SMALL]


def _plan_cases():
    return [c for c in G2.PLAN_CASES + G2.RANGE_CASES if c["id"].startswith("plan-") and not c.get("ab")]


@pytest.mark.parametrize("family", sorted(T.CONV3D))
def test_tile_edge_shapes_of_the_3d_suite_reach_no_hand_over_class(family):
    """the gap the many-tile shapes close: on SMALL no tile has both a predecessor and a successor, no column lies inside a range, no
    range crosses a batch element"""
    assert {T.ROUTE_FAMILY[c["route"]] for c in _small_cases()} == set(T.CONV3D)
    for dims in G3.SMALL:
        c = T.classes3d(family, dims)
        assert c["total"] <= 130 and c["len_max"] <= 2, (dims, c)
        assert (c["middle"], c["whole_inside"], c["cross_n"]) == (0, 0, 0), (dims, c)


def test_tile_edge_shapes_of_the_2d_suite_give_no_range_of_three_items():
    """PLAN_EDGE: at most 120 items against 512 slots -- one item per workgroup, two where the grid is rounded down to a multiple of 8; no
    item is both prefetched during its predecessor and followed by a successor"""
    for case in _plan_cases():
        fam = T.family2d(case["kern"], case["cout"])
        for shape in case["shapes"]:
            c = T.classes2d(fam, tuple(shape), case["cout"])
            assert c["total"] <= 120 and c["len_max"] <= 2 and c["G"] == T.grid(c["total"], T.CUS, 0, 2), (case["id"], shape, c)


@pytest.mark.parametrize("family", sorted(T.CONV3D))
def test_many_tile_shapes_reach_every_class_of_a_3d_family(family):
    keys = T.CLASSES_3D_PAIRS if T.CONV3D[family]["depth"] == "pairs" else T.CLASSES_3D
    counts = []
    for dims in T.ranges3d(family):
        per_shape = [T.classes3d(family, dims, reserved=r) for r in T.RESERVES]
        assert max(c["len_min"] for c in per_shape) >= 3, (dims, per_shape)
        assert per_shape[0]["G"] != per_shape[1]["G"], dims                    # (two different partitions of the same tiles)
        assert dims[0] * dims[1] * dims[2] * dims[3] <= 200000, dims
        counts += per_shape
    got = T.union(counts, keys)
    assert all(v > 0 for v in got.values()), got
    assert max(c["seg_max"] for c in counts) >= 3 and min(c["seg_min"] for c in counts) == 1


def test_many_tile_shapes_reach_every_successor_kind_of_a_2d_instance():
    """per kernel instance (conv2d_wino2: dilation x item width; conv2d_k3: NT x dilation) the union over its cases and both grids holds
    same-image, next-image and next-group successors, and every range of the reserve-128 grid has at least three items"""
    by_inst = {}
    for case in _plan_cases():
        fam = T.family2d(case["kern"], case["cout"])
        assert case["many"] == T.batch2d(fam, case["cout"], G2.MANY_HW), case["id"]          # the smallest batch that does it
        shape = (case["many"],) + G2.MANY_HW
        per_shape = [T.classes2d(fam, shape, case["cout"], reserved=r) for r in T.RESERVES]
        assert max(c["len_min"] for c in per_shape) >= 3, (case["id"], per_shape)
        by_inst.setdefault((case["kern"], fam), []).extend(per_shape)
    assert sorted(by_inst) == [("conv2d_k3_kernel<2, 1>", "k3_nt2"), ("conv2d_k3_kernel<2, 2>", "k3_nt2"), ("conv2d_k3_kernel<4, 1>", "k3_nt4"),
                               ("conv2d_k3_kernel<4, 2>", "k3_nt4"), ("conv2d_wino2_kernel<1>", "wino2"), ("conv2d_wino2_kernel<1>", "wino2_wide"),
                               ("conv2d_wino2_kernel<2>", "wino2"), ("conv2d_wino2_kernel<2>", "wino2_wide")]
    for inst, counts in by_inst.items():
        got = T.union(counts, T.CLASSES_2D)
        assert all(v > 0 for v in got.values()), (inst, got)
