"""A plain Python model of how the persistent convolution kernels split their tile list among workgroups.

Every 3x3x3 and NHWC 3x3 kernel launches ``G = grid(total, ...)`` workgroups (``estd_persistent_grid``, csrc/estd_common.h); workgroup
``r`` walks the contiguous range ``[total * r // G, total * (r + 1) // G)`` and runs a software pipeline inside it: the 3D kernels
over column segments (the same (n, h-tile, w-tile) over consecutive depth pairs / planes), the 2D kernels over items
(output-channel group, n, h-tile, w-tile), group-major, decoding item ``u + 1`` while they work on ``u``.  The hand-over between two
tiles of a range is where those pipelines can go wrong, and whether a shape reaches a hand-over at all depends only on this arithmetic.

``classes3d`` / ``classes2d`` count, for one launch, the kinds of range, segment and tile (3D) or successor pair (2D) it contains, so
that a test can say which of them its shapes reach.  The tables below copy what the launchers use (tests/test_tile_ranges_cpu.py reads
the same constants out of the sources).  ``RANGES_3D`` / ``RANGES_2D`` are the many-tile shapes of the GPU route suites: thin maps
(H = 9, W = 17: 2 x 2 tiles of 8 x 16, three of them ragged) with a large batch, so that a thousand tiles cost under 200 k voxels.
"""

CUS = 256                      # compute units of an MI355X
RESERVES = (0, 128)            # ops.set_reserved_cus: the full grid and the smallest one the library allows


# ----------------------------------------------------------------------------------------------------------------------- the grid
def grid(total, cus, reserved, per_cu):
    """estd_persistent_grid(total, per_cu) on a device of ``cus`` compute units under estd_set_reserved_cus(reserved)"""
    avail = cus - reserved
    slots = (avail if avail > 8 else 8) * per_cu               # estd_persistent_wgs
    g = total if total < slots else slots
    if g >= 8:
        g &= ~7
    return g


def ranges(total, G):
    """[(u, u_end)] of range r = 0 .. G - 1"""
    return [(total * r // G, total * (r + 1) // G) for r in range(G)]


def range_of_block(bid, G):
    """the range index workgroup ``bid`` takes: XCD x (blocks x, x + 8, ...) owns a contiguous block of ranges when G is a multiple of 8"""
    return (bid & 7) * (G >> 3) + (bid >> 3) if G % 8 == 0 else bid


# --------------------------------------------------------------------------------------------------------------------- the tables
# 3x3x3 kernels: tile height / width, depth steps per column ("pairs": ceil(D / 2), "planes": D), resident workgroups per CU
CONV3D = {
    "direct": dict(src="conv3d_mfma.hip", th=8, tw=16, depth="planes", per_cu=2),
    "wino3": dict(src="conv3d_wino3.hip", th=8, tw=16, depth="pairs", per_cu=1),
    "wino2": dict(src="conv3d_wino2.hip", th=8, tw=16, depth="pairs", per_cu=1),
    "wino2_c16": dict(src="conv3d_wino2_c16.hip", th=16, tw=16, depth="pairs", per_cu=1),
}
# route of tests/test_gpu_conv3d_routes.py -> the family of its persistent kernel (conv3d_xout_kernel is no persistent-range kernel)
ROUTE_FAMILY = {"direct": "direct", "wino3": "wino3", "wino3+xout": "wino3", "wino2": "wino2", "wino2_xout": "wino2", "wino2_o16": "wino2",
                "wino2_c16": "wino2_c16"}
# NHWC 3x3 kernels: tile height / width, output channels per group, resident workgroups per CU.  conv2d_wino2 takes 64-channel items of
# half the tile height where cout is a multiple of 64; conv2d_k3's group is 16 * NT channels.
CONV2D = {
    "wino2": dict(src="conv2d_wino2.hip", th=8, tw=16, group=32, per_cu=2),
    "wino2_wide": dict(src="conv2d_wino2.hip", th=4, tw=16, group=64, per_cu=2),
    "k3_nt2": dict(src="conv2d_mfma.hip", th=8, tw=16, group=32, per_cu=2),
    "k3_nt4": dict(src="conv2d_mfma.hip", th=8, tw=16, group=64, per_cu=2),
}


def family2d(kern, cout):
    """the CONV2D family of a kernel instance name as torch.profiler prints it (``conv2d_wino2_kernel<1>``, ``conv2d_k3_kernel<4, 2>``)"""
    if kern.startswith("conv2d_wino2_kernel"):
        return "wino2_wide" if cout % 64 == 0 else "wino2"
    if kern.startswith("conv2d_k3_kernel"):
        return "k3_nt%s" % kern[len("conv2d_k3_kernel<")]
    raise KeyError(kern)


def _cdiv(a, b):
    return (a + b - 1) // b


def geometry3d(family, dims):
    """-> (tiles_h, tiles_w, tiles per depth column, total tiles) of the family's launcher for an (N, D, H, W) batch"""
    N, D, H, W = dims
    f = CONV3D[family]
    tiles_h, tiles_w = _cdiv(H, f["th"]), _cdiv(W, f["tw"])
    col = _cdiv(D, 2) if f["depth"] == "pairs" else D
    return tiles_h, tiles_w, col, N * tiles_h * tiles_w * col


def decode3d(family, dims, u):
    """tile u -> (n, h-tile, w-tile, depth step), as the kernels' segment header decodes it"""
    tiles_h, tiles_w, col, _ = geometry3d(family, dims)
    c, dp = divmod(u, col)
    c2, twi = divmod(c, tiles_w)
    n, thi = divmod(c2, tiles_h)
    return n, thi, twi, dp


def geometry2d(family, shape, cout):
    """-> (groups, tiles_h, tiles_w, total items) of the family's launcher for an (N, H, W) batch"""
    N, H, W = shape
    f = CONV2D[family]
    tiles_h, tiles_w = _cdiv(H, f["th"]), _cdiv(W, f["tw"])
    groups = cout // f["group"]
    return groups, tiles_h, tiles_w, groups * N * tiles_h * tiles_w


def decode2d(family, shape, cout, item):
    """item -> (group, n, h-tile, w-tile): the ``decode`` lambda of conv2d_wino2 / conv2d_k3 (group-major)"""
    _, tiles_h, tiles_w, _ = geometry2d(family, shape, cout)
    grp, t = divmod(item, shape[0] * tiles_h * tiles_w)
    t, twi = divmod(t, tiles_w)
    n, thi = divmod(t, tiles_h)
    return grp, n, thi, twi


# ----------------------------------------------------------------------------------------------------------------- classification
CLASSES_3D = ("only", "first", "middle", "last", "whole_inside", "cross_n", "longer_than_column")
CLASSES_3D_PAIRS = CLASSES_3D + ("odd_last_start",)       # only the depth-pair kernels have a last pair of one plane
CLASSES_2D = ("same_image", "next_image", "next_group")


def classes3d(family, dims, cus=CUS, reserved=0):
    """Counts over one launch of a 3x3x3 kernel:
      total, G             tiles and workgroups
      len_min, len_max     tiles per range
      seg_min, seg_max     column segments per range
      only / first / middle / last   tiles by their place in their segment (only: a segment of one tile; middle: a predecessor AND a
                           successor in the segment -- both hand-overs of the pipeline)
      whole_inside         complete columns strictly inside a range (tiles of the range before and after them)
      cross_n              ranges whose first and last tile lie in different batch elements
      longer_than_column   ranges with more tiles than a column has
      odd_last_start       (depth-pair kernels) ranges that start on the one-plane last pair of an odd D"""
    _, _, col, total = geometry3d(family, dims)
    tiles_per_n = total // dims[0]
    f = CONV3D[family]
    G = grid(total, cus, reserved, f["per_cu"])
    c = dict(total=total, G=G, len_min=total, len_max=0, seg_min=total, seg_max=0)
    c.update({k: 0 for k in (CLASSES_3D_PAIRS if f["depth"] == "pairs" else CLASSES_3D)})
    for u, e in ranges(total, G):
        n_seg, a = 0, u
        while a < e:                                           # the kernels' ``while (u < u_end)`` over column segments
            b = min(e, (a // col + 1) * col)
            n_seg += 1
            if b - a == 1:
                c["only"] += 1
            else:
                c["first"] += 1
                c["last"] += 1
                c["middle"] += b - a - 2
            if b - a == col and a > u and b < e:
                c["whole_inside"] += 1
            a = b
        c["len_min"], c["len_max"] = min(c["len_min"], e - u), max(c["len_max"], e - u)
        c["seg_min"], c["seg_max"] = min(c["seg_min"], n_seg), max(c["seg_max"], n_seg)
        if e > u:
            c["cross_n"] += u // tiles_per_n != (e - 1) // tiles_per_n
            c["longer_than_column"] += e - u > col
            if f["depth"] == "pairs":
                c["odd_last_start"] += dims[1] % 2 == 1 and u % col == col - 1
    return c


def classes2d(family, shape, cout, cus=CUS, reserved=0):
    """Counts over one launch of an NHWC 3x3 kernel: total, G, len_min, len_max, and the successor pairs (u, u + 1) inside a range by
    what changes from an item to the one the kernel prefetches during it: same_image (only the tile), next_image (the input descriptor),
    next_group (the weight stream and the folded scale / shift)"""
    groups, tiles_h, tiles_w, total = geometry2d(family, shape, cout)
    per_image = tiles_h * tiles_w
    per_group = shape[0] * per_image
    G = grid(total, cus, reserved, CONV2D[family]["per_cu"])
    c = dict(total=total, G=G, len_min=total, len_max=0, same_image=0, next_image=0, next_group=0)
    for u, e in ranges(total, G):
        c["len_min"], c["len_max"] = min(c["len_min"], e - u), max(c["len_max"], e - u)
        for i in range(u, e - 1):
            if i // per_group != (i + 1) // per_group:
                c["next_group"] += 1
            elif i // per_image != (i + 1) // per_image:
                c["next_image"] += 1
            else:
                c["same_image"] += 1
    return c


def union(counts, keys):
    """sum of each class over several launches"""
    return {k: sum(c[k] for c in counts) for k in keys}


# ------------------------------------------------------------------------------------------------------ the many-tile test shapes
# (N, D, H, W).  Short odd columns (3 depth pairs, the last of one plane; 5 planes for the direct kernel): ranges of 5-6 tiles hold whole
# columns, cross batch elements and start on the odd last pair.  Long odd columns (21 pairs / 41 planes): many middle tiles per segment.
RANGES_3D = [(120, 5, 9, 17), (14, 41, 9, 17)]
# the stereo-head kernel's tiles are 16 x 16: H = 17 gives it the 2 x 2 ragged tiles per volume again (its inputs have 16 channels)
RANGES_3D_C16 = [(120, 5, 17, 17), (14, 41, 17, 17)]


def ranges3d(family):
    return RANGES_3D_C16 if family == "wino2_c16" else RANGES_3D


def batch2d(family, cout, hw=(9, 17), min_len=3):
    """the smallest batch N >= 3 at which, on ``hw`` maps, every range of the reserve-128 grid holds at least ``min_len`` items and the
    two grids together contain every successor kind the layer can have.  next_group needs THREE groups: G is even, so the one boundary
    between two groups (item total / 2) is always a range boundary as well."""
    groups = cout // CONV2D[family]["group"]
    want = [k for k in CLASSES_2D if k != "next_group" or groups > 2]
    for n in range(3, 4096):
        cs = [classes2d(family, (n,) + tuple(hw), cout, reserved=r) for r in RESERVES]
        if max(c["len_min"] for c in cs) >= min_len and all(v > 0 for v in union(cs, want).values()):
            return n
    raise ValueError((family, cout))
