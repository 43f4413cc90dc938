"""CPU: the numpy reference of the global registration (tests/global_reg_ref.py) held against itself, so that the GPU suites compare the
kernels with something that has been checked: the invariances of the descriptors, the mixer against tests/mesh_sample_ref.py's, the
exact matcher against the candidate-based one, every status of the hypotheses, and the whole chain on the fixture.

The chain: about 3 000 points per side after thinning at 7 cm, DISJOINT samples of the scene on the two sides (other seeds), three
motions -- 90 degrees about z and 1 m, 175 degrees about a skew axis and 3 m, one drawn from a seed.  The global stage ALONE must land
inside 98 mm and 5 degrees, the start from which tests/test_gpu_registration.py's x10 case shows the staged ``register`` converging: a
condition on the fixture, not on the code under test (a reference that missed it would call for another scene or voxel, never for
another bar).  The figures are printed (GLOBAL-REG-REF lines; recorded in profiles/global_register_gpu_tests.txt)."""
import numpy as np
import pytest

import global_reg_ref as G
import mesh_sample_ref as MS


@pytest.fixture(scope="module")
def cloud():
    """the part of the thinned target around the first box: floor, five faces, their edges and corners"""
    fx = G.fixture("z90")
    p = fx["tgt"]
    near = (np.abs(p[:, 0] - 0.8) < 0.65) & (np.abs(p[:, 1] - 0.7) < 0.6)
    assert 400 <= near.sum() <= 900
    return p[near].copy(), fx["tgt_normal"][near].copy()


def test_the_scene_is_a_mesh_of_a_few_hundred_triangles_without_symmetry():
    xyz, faces = G.scene_mesh()
    assert 200 <= faces.shape[0] <= 500 and faces.min() == 0 and faces.max() == xyz.shape[0] - 1
    sizes = [b[0] for b in G.BOXES]
    yaws = [b[1] for b in G.BOXES]
    assert len({tuple(sorted(s)) for s in sizes}) == 3 and len({abs(y) for y in yaws}) == 3
    # the normals point into the room: from the floor up, from the two walls inwards
    import rigid_align_ref as RA
    n, area = RA.face_normals(xyz, faces)
    assert (n[:2, 2] > 0.99).all() and (n[2:4, 0] > 0.99).all() and (n[4:6, 1] > 0.99).all() and (area > 0).all()
    # no rigid symmetry: the second moments about the centroid of the area have three well separated eigenvalues
    c = xyz[faces].mean(1)
    mean = (c * area[:, None]).sum(0) / area.sum()
    ev = np.linalg.eigvalsh(((c - mean).T * area) @ (c - mean) / area.sum())
    assert ev[1] / ev[0] > 1.2 and ev[2] / ev[1] > 1.2, ev


def test_the_mixer_is_mesh_sample_refs():
    r = G.ransac(np.random.RandomState(0).rand(50, 3), np.random.RandomState(1).rand(50, 3), 16, 12345, 0.1, 0.0)
    assert r["status"].shape == (16,)
    for seed, h, j in ((0, 0, 0), (12345, 7, 2), (2 ** 64 - 1, 2 ** 31 - 1, 1)):
        assert int(MS.h64(seed, np.asarray([h], np.uint64), j)[0]) == MS.h64_int(seed, h, j)


def test_descriptors_do_not_change_under_a_rigid_motion(cloud):
    p, n = cloud
    T = G.motion("skew175")
    q = (p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    m = (n.astype(np.float64) @ T[:3, :3].T).astype(np.float32)
    for oriented in (True, False):
        a, b = G.descriptors(p, n, 16, 0.3, oriented), G.descriptors(q, m, 16, 0.3, oriented)
        same_lists = (a["index"] == b["index"]).all(1)
        moved = np.abs(a["hist"][same_lists].astype(np.int64) - b["hist"][same_lists]).sum() / 2
        share = moved / max(1, 3 * a["pairs"][same_lists].sum())
        print("GLOBAL-REG-REF invariance oriented=%s: %d of %d rows keep their neighbour lists; %.3g of their binned features move a bin "
              "under the motion's rounding" % (oriented, same_lists.sum(), p.shape[0], share))
        assert same_lists.mean() > 0.9 and (a["pairs"][same_lists] == b["pairs"][same_lists]).all()
        assert share < 1e-2


def test_the_folded_descriptor_ignores_the_sign_of_every_normal(cloud):
    p, n = cloud
    flip = np.where(np.random.RandomState(4).rand(n.shape[0]) < 0.5, -1.0, 1.0).astype(np.float32)
    a, b = G.descriptors(p, n, 16, 0.3, False), G.descriptors(p, n * flip[:, None], 16, 0.3, False)
    assert (a["hist"] == b["hist"]).all() and (a["pairs"] == b["pairs"]).all() and (a["valid"] == b["valid"]).all()
    assert a["desc"].tobytes() == b["desc"].tobytes()
    c = G.descriptors(p, n * flip[:, None], 16, 0.3, True)
    assert (a["hist"] != c["hist"]).any()                                   # the oriented one does not
    for g in range(3):
        s = a["desc"][a["valid"] == 1][:, 11 * g:11 * g + 11].astype(np.float64).sum(1)
        assert np.abs(s - 1).max() < 1e-6


def test_the_two_matchers_agree(cloud):
    p, n = cloud
    d = G.descriptors(p, n, 16, 0.3)["desc"]
    a, b = d[:150], d[150:].copy()
    b[7] = b[3]                                                             # duplicated target rows: the smallest index wins
    b[200] = b[3]
    a[0] = b[3]
    av = (np.arange(150) % 11 != 0).astype(np.uint8)
    av[0] = 1
    bv = (np.arange(b.shape[0]) % 7 != 1).astype(np.uint8)
    bv[[3, 7, 200]] = 1
    slow, fast = G.match(a, b, av, bv), G.match_fast(a, b, av, bv)
    for x, y in zip(slow, fast):
        assert x.tobytes() == y.tobytes()
    first = int(np.nonzero((b == b[3]).all(1) & (bv == 1))[0][0])
    assert first <= 3 and slow[0][0] == first and slow[1][0] == 0 and slow[2][0] == 0
    assert (slow[0][av == 0] == -1).all() and np.isinf(slow[1][av == 0]).all() and bv[slow[0][av == 1]].all()
    none = G.match(a, b, None, np.zeros(b.shape[0], np.uint8))
    assert (none[0] == -1).all() and np.isinf(none[1]).all() and np.isinf(none[2]).all()


def test_every_status_is_produced():
    rng = np.random.RandomState(2)
    P = rng.rand(40, 3).astype(np.float32)
    T = G.motion("z90")
    Q = (P.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    r = G.ransac(P, Q, 512, 3, 0.01, 0.9)
    assert set(np.unique(r["status"])) == {0, 1} and r["best_count"] == 40 and (r["count"][r["status"] == 0] == 40).all()
    assert G.error(G.winner_T(r), T)[0] < 1e-5
    r = G.ransac(P, Q * np.float32(2.0), 64, 3, 0.01, 0.9)
    assert set(np.unique(r["status"])) <= {1, 2} and r["hypothesis"] == -1
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = np.arange(40)
    r = G.ransac(line, line, 64, 3, 0.01, 0.9)
    assert set(np.unique(r["status"])) <= {1, 3} and (r["status"] == 3).any() and (r["T"] == 0).all()
    assert (G.ransac(P[:0], Q[:0], 8, 0, 0.1, 0.9)["status"] == 1).all()


@pytest.mark.parametrize("name", G.MOTIONS)
def test_the_reference_chain_lands_inside_the_basin(name):
    fx = G.fixture(name)
    assert 2400 <= fx["src"].shape[0] <= 3600 and 2400 <= fx["tgt"].shape[0] <= 3600
    out = G.chain(fx["src"], fx["src_normal"], fx["tgt"], fx["tgt_normal"])
    et, er = G.error(out["T_global"], fx["T_true"])
    e0, r0 = G.error(np.eye(4), fx["T_true"])
    print("GLOBAL-REG-REF chain %s: %d and %d points, start %.0f mm %.1f deg; %d mutual pairs, winner %d with %d inliers (fitness %.3f), "
          "tallies %s; global stage alone %.1f mm %.2f deg" % (name, fx["src"].shape[0], fx["tgt"].shape[0], 1e3 * e0, np.degrees(r0), out["pairs"],
                                                              out["hypothesis"], out["count"], out["fitness"],
                                                              np.bincount(out["ransac"]["status"], minlength=4).tolist(), 1e3 * et, np.degrees(er)))
    assert out["reason"] == "global"
    assert et <= G.BASIN_T and er <= G.BASIN_R
