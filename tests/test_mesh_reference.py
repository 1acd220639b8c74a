"""The mesh voxelisers' fp64 reference (tests/_mesh_ref.py) against closed forms, and the oracle (oracle/xlb_numpy.py,
oracle/mesh_bc.py: what the HIP kernels equal bit for bit) against that reference.  The oracle was written from the kernels, so
only a restatement that shares nothing with either can catch a mistake present in both: the AABB loop window that started one
cell too low (false solid voxels next to acute corners) is the case in point, and the AABB cases below fail on it.

The oracle's pure-Python loops set the size of this module: it runs on the zoo members it can afford, the cross of all methods,
both lattices and close_voxels 1, 2, 3 on the small ones.  The GPU module covers the rest of the zoo with the kernels."""

import functools

import numpy as np
import pytest

import _mesh_ref as mr
from oracle import mesh_bc as mb
from oracle import xlb_numpy as orc

from _util import icosphere, mesh_zoo

ZOO = mesh_zoo()
ZOO["sphere1"] = (icosphere((4.43, 4.87, 3.91), 2.63, 1), (9, 10, 8))  # 80 triangles: the sphere the oracle can afford
BC_ID = 3
ALL = [("AABB", 0), ("RAY", 0), ("WINDING", 0), ("AABB_CLOSE", 1), ("AABB_CLOSE", 2), ("AABB_CLOSE", 3)]
CASES = [(name, lattice, method, h) for name in ("box_low_faces", "box_high_faces", "plate", "box") for lattice in ("D3Q19", "D3Q27") for method, h in ALL]
CASES += [("two_boxes", "D3Q19", m, h) for m, h in ALL[:3] + [ALL[4]]]
CASES += [("box_zero_area", "D3Q19", m, h) for m, h in ALL[:4]]
CASES += [("sphere1", "D3Q27", m, h) for m, h in ALL[:3] + [ALL[5]]]
CLOSED = ["torus", "box", "box_low_faces", "box_high_faces", "two_boxes", "box_zero_area", "sphere1"]


@functools.lru_cache(maxsize=None)
def reference(name):
    verts, shape = ZOO[name]
    return mr.MeshReference(verts, shape)


@functools.lru_cache(maxsize=None)
def oracle_masks(name, lattice, method, h):
    verts, shape = ZOO[name]
    lat = orc.Lattice(lattice)
    z1, zq, d0 = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool), np.zeros((lat.q,) + shape, np.float32)
    if method == "AABB":
        return orc.mesh_mask_aabb(shape, lat, BC_ID, verts, z1, zq) + (None,)
    if method == "RAY":
        return mb.mesh_mask_ray(shape, lat, BC_ID, verts, z1, zq, d0)
    if method == "WINDING":
        return mb.mesh_mask_winding(shape, lat, BC_ID, verts, z1, zq, d0)
    return mb.mesh_mask_aabb_close(shape, lat, BC_ID, verts, h, z1, zq, d0)


# ---- the reference against closed forms ------------------------------------------------------------------------------
def test_box_axis_links_are_the_distance_to_the_face():
    lo, hi = np.array([2.31, 3.43, 1.63]), np.array([6.27, 7.79, 5.41])
    shape = (9, 10, 8)
    cells = np.argwhere(np.ones(shape, bool))
    axis = np.array([d for d in mr.DIRS26 if np.abs(d).sum() == 1])
    cut, amb, t, ok = mr.link_hits(mr.box(lo, hi), cells + 0.5, axis)[1.0]
    lo, hi = np.float32(lo).astype(np.float64), np.float32(hi).astype(np.float64)
    assert not amb.any() and np.array_equal(cut, ok)
    p = cells + 0.5
    for i, d in enumerate(axis):
        a = int(np.flatnonzero(d)[0])
        inside = np.all([(p[:, b] > lo[b]) & (p[:, b] < hi[b]) for b in range(3) if b != a], axis=0)
        s = np.stack([(lo[a] - p[:, a]) * d[a], (hi[a] - p[:, a]) * d[a]])  # ray parameters of the two faces across the link
        valid = inside & (s >= 0) & (s <= 1)
        assert np.array_equal(cut[i], valid.any(axis=0))
        assert np.array_equal(t[i][cut[i]], np.where(valid, s, np.inf).min(axis=0)[cut[i]])  # exactly: face - centre
    assert cut.sum() > 150


def test_sphere_hits_lie_between_inscribed_and_circumscribed_radius():
    ctr, rad = np.array([8.83, 7.87, 6.91]), 4.23
    verts = icosphere(ctr, rad, 2)
    tri = verts.astype(np.float64).reshape(-1, 3, 3)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = np.abs(np.einsum("tk,tk->t", tri[:, 0] - ctr, nrm / np.linalg.norm(nrm, axis=1, keepdims=True))).min()
    r_out = np.linalg.norm(tri - ctr, axis=2).max()
    assert 0.95 * rad < r_in < r_out < rad * (1 + 1e-6)
    cells = np.argwhere(np.ones((18, 16, 14), bool))
    cut, amb, t, ok = mr.link_hits(verts, cells + 0.5)[1.0]
    assert cut.sum() > 3000
    for i, d in enumerate(mr.DIRS26):
        sel = ok[i]
        hit = cells[sel] + 0.5 + t[i][sel, None] * d / np.linalg.norm(d)
        r = np.linalg.norm(hit - ctr, axis=1)
        assert np.all((r >= r_in - 1e-9) & (r <= r_out + 1e-9))
        # and the ends of a cut link lie on the two sides of that shell, or inside it
        r0, r1 = np.linalg.norm(cells[cut[i]] + 0.5 - ctr, axis=1), np.linalg.norm(cells[cut[i]] + 0.5 + d - ctr, axis=1)
        assert np.all((np.minimum(r0, r1) <= r_out) & (np.maximum(r0, r1) >= r_in))


@pytest.mark.parametrize("name", ["sphere1", "torus", "box", "two_boxes"])
def test_winding_number_is_one_inside_zero_outside(name):
    verts, shape = ZOO[name]
    ref = reference(name)
    w = ref.winding[ref.window]
    assert np.abs(w - np.round(w)).max() < 1e-12 and set(np.round(w).astype(int)) == {0, 1}
    wi = mr.winding_numbers(mr.inward(verts), np.argwhere(ref.window) + 0.5)
    assert np.abs(wi + w).max() < 1e-12  # inward orientation: -1 inside


def test_separation_of_a_voxel_from_one_triangle_by_hand():
    low = np.zeros((1, 3))
    # a box axis: the triangle lies in 1.25 <= x <= 1.5 over the middle of the voxel
    assert mr.tri_box_separation([[1.25, 0.2, 0.2], [1.5, 0.8, 0.3], [1.3, 0.4, 0.9]], low)[0] == pytest.approx(0.25, abs=1e-15)
    assert mr.tri_box_separation([[0.3, 0.2, -0.5], [0.4, 0.8, -0.125], [0.7, 0.4, -0.3]], low)[0] == pytest.approx(0.125, abs=1e-15)
    # the normal: a large triangle in the plane x + y + z = 3.3 above the corner (1, 1, 1), 0.3 / sqrt(3) away
    big = np.array([[3.3, 0.0, 0.0], [0.0, 3.3, 0.0], [0.0, 0.0, 3.3]]) + np.array([[4.0, -2.0, -2.0], [-2.0, 4.0, -2.0], [-2.0, -2.0, 4.0]])
    assert mr.tri_box_separation(big, low)[0] == pytest.approx(0.3 / 3**0.5, abs=1e-14)
    # an edge cross product: the edge A B (direction (-1, 1, 0.75)) passes the voxel's edge x = y = 1 at x + y = 2.2; the axis
    # (A B) x e_z = (1, 1, 0) / sqrt(2) sees a gap of 0.2 / sqrt(2), every box axis and the normal see an overlap
    tri = np.array([[1.5, 0.7, 0.125], [0.7, 1.5, 0.725], [1.6, 1.6, 0.5]])
    assert mr.tri_box_separation(tri, low)[0] == pytest.approx(0.2 / 2**0.5, abs=1e-14)
    ax = mr.tri_box_axes(tri)
    assert len(ax) == 13 and np.allclose(np.linalg.norm(ax, axis=1), 1.0)
    seps = [mr.tri_box_separation(tri, low)[0]] + [max((tri @ a).min() - (0.5 * a.sum() + 0.5 * np.abs(a).sum()), (0.5 * a.sum() - 0.5 * np.abs(a).sum()) - (tri @ a).max()) for a in ax[:4]]
    assert all(s < 0 for s in seps[1:])
    # moved by (-0.3, -0.3, 0) it overlaps; an exact contact (a triangle in the plane of a face) counts as overlap of the closed box
    assert mr.tri_box_separation(tri - [0.3, 0.3, 0.0], low)[0] < 0
    assert mr.tri_box_separation([[0.0, 0.2, 0.2], [0.0, 0.8, 0.3], [0.0, 0.4, 0.9]], low)[0] == 0.0
    solid, amb = mr.surface_voxels(np.float32([[0.0, 0.2, 0.2], [0.0, 0.8, 0.3], [0.0, 0.4, 0.9]]), (-1, 0, 0), (1, 1, 1))
    assert solid.all() and not amb.any()


def test_closing_fills_a_shell_and_copies_the_border():
    a = np.zeros((16, 16, 16), bool)
    a[5:11, 5:11, 5:11] = True
    a[6:10, 6:10, 6:10] = False  # a shell with a 4^3 cavity, 2 h = 4 cells from the faces as the padding guarantees
    a[0, 1, 1] = a[15, 15, 15] = True  # voxels on the grid's border
    one, two = mr.close_padded(a, 1), mr.close_padded(a, 2)
    assert not one[6:10, 6:10, 6:10].any() and two[6:10, 6:10, 6:10].all()  # a 3^3 cube fits into the cavity, a 5^3 cube does not
    assert (one | ~a).all() and (two | ~a).all()  # extensive
    assert two[0, 1, 1] and two[15, 15, 15] and not two[2, 2, 2] and not two[1, 1, 1]  # the border is copied, not filtered
    assert two.sum() == a.sum() + 4**3


# ---- the oracle against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lattice,method,h", CASES)
def test_oracle_vs_reference(name, lattice, method, h):
    lat = orc.Lattice(lattice)
    req, amb, stats = reference(name).masks(method, lat.c, BC_ID, h)
    mr.check_caps(stats)
    got_bc, got_mm, got_d = oracle_masks(name, lattice, method, h)
    dis = mr.disagreements(req, amb, got_bc, got_mm, got_d)
    print(name, lattice, method, h, stats, dis)
    assert dis["bc"] == 0 and dis["mm"] == 0 and dis["dist"] == 0, dis
    assert not got_bc[0][~reference(name).window].any() and not got_mm[:, ~reference(name).window].any()
    if method == "WINDING" and name == "plate":
        assert not got_bc.any() and not got_mm.any()  # no centre inside: nothing solid, nothing tagged


def test_oracle_distance_deviation_is_what_the_tolerance_was_taken_from():
    """DIST_TOL = 4 x the largest |oracle - reference| over all cases above; this is where the figure is measured."""
    worst, where = 0.0, None
    for name, lattice, method, h in CASES:
        if method == "AABB":
            continue
        req, amb, _ = reference(name).masks(method, orc.Lattice(lattice).c, BC_ID, h)
        dev = mr.disagreements(req, amb, *oracle_masks(name, lattice, method, h))["dist_max"]
        if dev > worst:
            worst, where = dev, (name, lattice, method, h)
    print("largest |oracle - fp64 reference| of a wall distance: %.3e at %s; DIST_TOL = %.3e" % (worst, where, mr.DIST_TOL))
    assert 0.5 * mr.DIST_MEASURED < worst <= mr.DIST_MEASURED


@pytest.mark.parametrize("name", ["sphere1", "box"])
def test_inward_orientation_and_zero_area_triangles_change_nothing_but_winding(name):
    verts, shape = ZOO[name]
    lat = orc.Lattice("D3Q27")
    a, b = reference(name), mr.MeshReference(mr.with_zero_area_triangle(mr.inward(verts)), shape)
    for method, h in (("AABB", 0), ("RAY", 0), ("AABB_CLOSE", 2)):
        ra, aa, _ = a.masks(method, lat.c, BC_ID, h)
        rb, ab, _ = b.masks(method, lat.c, BC_ID, h)
        for k in ("bc", "mm"):
            assert np.array_equal(ra[k], rb[k]) and np.array_equal(aa[k], ab[k])
        if ra["dist"] is not None:  # (another vertex order: another fp64 rounding)
            assert np.array_equal(aa["dist"], ab["dist"]) and np.abs(ra["dist"] - rb["dist"]).max() < 1e-12
    rw, aw, _ = b.masks("WINDING", lat.c, BC_ID)
    assert not rw["bc"].any() and not rw["mm"].any() and not aw["bc"].any()


@pytest.mark.parametrize("name", CLOSED)
@pytest.mark.parametrize("lattice", ["D3Q19", "D3Q27"])
def test_winding_is_watertight(name, lattice):
    """On a closed mesh every link from a solid voxel to a fluid one crosses the surface: the fluid voxel carries the id and
    missing[l], except through ambiguous links."""
    lat = orc.Lattice(lattice)
    req, amb, stats = reference(name).masks("WINDING", lat.c, BC_ID)
    mr.check_caps(stats)
    solid = req["bc"] == mr.BC_SOLID
    outputs = [(req["bc"], req["mm"])]
    if (name, lattice, "WINDING", 0) in CASES:
        o = oracle_masks(name, lattice, "WINDING", 0)
        outputs.append((o[0][0], o[1]))
    links = 0
    for l in range(lat.q):
        c = tuple(int(x) for x in lat.c[:, l])
        if not any(c):
            continue
        src = mr._shift(solid, tuple(-x for x in c))  # solid at x - c_l
        through = ~solid & src & ~amb["mm"][l]
        links += int(through.sum())
        for bc, mm in outputs:
            assert mm[l][through].all() and (bc[through] == BC_ID).all()
    print(name, lattice, "solid-to-fluid links:", links, "untagged: 0")
    assert links > 200


def test_integer_box_is_left_to_the_oracle():
    """Every face of this box lies on a lattice plane: most of its voxels and links sit on a decision boundary, which is why it is
    compared with the oracle alone (GPU module) and never with this reference."""
    verts, shape = ZOO["integer_box"]
    ref = mr.MeshReference(verts, shape)
    _, _, stats = ref.masks("RAY", orc.Lattice("D3Q27").c, BC_ID)
    assert stats["amb_links"] > mr.LINK_CAP * stats["cut_links"]
