"""Where a test scene lies in the world.  A plain helper module of the test suite (not a conftest); numpy only.

Every case builder of the 3D back end places its scene within a few metres of the world origin.  A ``place`` moves the whole scene -- the
surfaces, the cameras, a volume's origin, a grid's corner -- by one rigid motion W of the world: the offset (d, -d, d / 2) metres and,
for the rotated placement, a fixed rotation about no coordinate axis first, so that gravity lies along no axis and no coordinate is small.
A placed scene is BUILT at its placement: the float64 geometry is moved in float64 and rounded to fp32 once.  Nothing adds an offset to
fp32 data.

``place`` is None (the builders' present scene, bit for bit) or a hashable pair (d, rotated), so that the cached builders can take it.
"""
import numpy as np

DISTANCES = (0, 8, 64, 512)
ROTATED_AT = 64
PLACES = {"d0": (0, False), "d8": (8, False), "d64": (64, False), "d64-rotated": (64, True), "d512": (512, False)}
FAMILY_PLACES = {"d64": (64, False), "d512": (512, False)}          # one placed case per kernel family at each
AXIS, ANGLE = (1.0, 2.0, 3.0), 0.7                                    # the rotated placement: 0.7 rad about (1, 2, 3) / sqrt(14)


def rotation():
    """the fixed rotation of the rotated placement, float64 [3,3] (Rodrigues); no entry is 0 or +-1"""
    a = np.asarray(AXIS, np.float64) / np.linalg.norm(AXIS)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(ANGLE) * Kx + (1.0 - np.cos(ANGLE)) * (Kx @ Kx)


def offset(d):
    return np.array([d, -d, d / 2.0], np.float64)


def matrix(place):
    """the rigid motion W of the world for ``place`` -> float64 [4,4] (the identity for None)"""
    W = np.eye(4)
    if place is not None:
        d, rotated = place
        if rotated:
            W[:3, :3] = rotation()
        W[:3, 3] = offset(d)
    return W


def points(p, place):
    """float64 points [..., 3] moved to ``place``, float64 (the caller rounds once)"""
    W = matrix(place)
    return np.asarray(p, np.float64) @ W[:3, :3].T + W[:3, 3]


def vectors(v, place):
    """float64 directions [..., 3] (normals) turned to ``place``"""
    return np.asarray(v, np.float64) @ matrix(place)[:3, :3].T


def pose(P, place):
    """a camera-to-world pose (or any [..., 4, 4] stack of them) of the unplaced scene -> the same camera in the placed world, W P"""
    return matrix(place) @ np.asarray(P, np.float64)


def conjugated(T, place):
    """a rigid motion of the unplaced world -> the same motion of the placed world, W T W^-1"""
    W = matrix(place)
    return W @ np.asarray(T, np.float64) @ np.linalg.inv(W)


def key(place):
    """None for the unplaced scene ((0, False) included: the builders' present data, bit for bit), else the hashable pair"""
    if place is None or (place[0] == 0 and not place[1]):
        return None
    return (place[0], bool(place[1]))


def label(place):
    return "d0" if place is None else "d%g%s" % (place[0], "-rotated" if place[1] else "")
