"""A plain fp64 restatement of the geometry behind the four mesh voxelisers (AABB, RAY, WINDING, AABB_CLOSE) and the wall
distances they hand to HybridBC, for the tests to compare kernels and oracle against.  NumPy only; it imports neither the
kernels' package nor oracle/, and follows none of their fp32 operation orders: the segment / triangle test is three dot
products with per-triangle vectors, the box / triangle test is the full 13-axis separating-axis test, and the closing is a
separable filter.

Every answer comes with an *ambiguous* mask: where the fp64 geometry is closer to a decision boundary than fp32 rounding can
be trusted (EPS, EPS_BOX, EPS_WIND below), nothing is required of the code under test.  What depends on an ambiguous voxel or
link is ambiguous too.  The shares of ambiguous links and voxels are capped by the tests (LINK_CAP, VOXEL_CAP), so a mesh
cannot hide behind its ambiguity.

Conventions (lattice units): voxel i spans [i, i + 1], its centre is i + 0.5; a mesh is a (3 n, 3) float32 triangle soup,
counter-clockwise seen from outside; `c` is the (3, q) integer array of lattice directions (passed in as data)."""

import numpy as np

BC_SOLID = 255
EPS = 1e-4  # links: margin in barycentric coordinates / ray parameter below which a hit is neither required nor forbidden
EPS_BOX = 1e-5  # voxels: |separation| (cells, normalised axes) below which an overlap is neither required nor forbidden
EPS_WIND = 1e-6  # winding number: distance from the 0.5 threshold
PARALLEL = 1e-3  # |d . n| below which a link counts as parallel to a triangle's plane
LINK_CAP = 0.05  # ambiguous links <= 5 % of the cut links of a case
VOXEL_CAP = 0.02  # ambiguous AABB voxels <= 2 % of the solid voxels of a case
# Largest |oracle - this reference| over every wall distance of tests/test_mesh_reference.py (measured and printed there by
# test_oracle_distance_deviation_is_what_the_tolerance_was_taken_from): 2.13e-6, on the rotated box under RAY, whose triangles
# are 9 cells long.  A different but equally valid fp32 order of a Moeller-Trumbore evaluation at coordinates <= 32 cannot
# move further than a few times that; a wrong triangle or a wrong link length moves a weight by 1e-2 or more.  The bound is
# 4 x the measurement.  The kernels get the same bound; it is never derived from their output.
DIST_MEASURED = 2.14e-6
DIST_TOL = 4 * DIST_MEASURED

DIRS26 = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], int)


# ---- segment against triangle --------------------------------------------------------------------------------------
def _triangles(verts):
    """(T, 3, 3) fp64 triangles of a soup, zero-area ones (which no segment can hit and no box test counts) dropped"""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return v[np.linalg.norm(n, axis=1) > 1e-9]


def link_hits(verts, centres, dirs=DIRS26, factors=(1.0,), eps=EPS, chunk=512):
    """Segments p + t d, 0 <= t <= factor |c|, d = c / |c|, from every centre p along every direction c against all triangles.
    Per triangle the margin is m = min(u, w, 1 - u - w, t, t_max - t) (barycentric coordinates of the plane crossing and the
    ray parameter).  Returns {factor: (cut, amb, t, t_ok)}, each (n_dirs, n_centres):
      cut   some triangle has m > eps;   amb: no such triangle, but one with m > -eps
      t     ray parameter of the closest candidate (m > -eps), inf without one
      t_ok  the link is cut and that closest candidate is itself robust (m > eps)
    A triangle (nearly) parallel to the link cannot be crossed robustly: it is out of the picture when the start point is
    further from its plane than the link can reach at that slope, and an ambiguous candidate otherwise."""
    tri = _triangles(verts)
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, int).reshape(-1, 3)
    out = {f: tuple(np.zeros((len(dirs), len(centres)), k) for k in (bool, bool, np.float64, bool)) for f in factors}
    for f in factors:
        out[f][2][:] = np.inf
    if len(tri) == 0 or len(centres) == 0:
        return out
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = np.cross(e1, e2)
    nhat = n / np.linalg.norm(n, axis=1, keepdims=True)
    for a in range(0, len(centres), chunk):
        tv = centres[a : a + chunk, None, :] - v0[None]  # (C, T, 3)
        plane = np.abs(np.einsum("ctk,tk->ct", tv, nhat))  # distance of the start point from each triangle's plane
        rows = np.arange(tv.shape[0])
        for i, c in enumerate(dirs):
            ln = float(np.sqrt(c @ c))
            d = c / ln
            par = np.abs(nhat @ d) < PARALLEL
            det = -(n @ d)
            det = np.where(par, 1.0, det)
            u = np.einsum("ctk,tk->ct", tv, np.cross(d, e2) / det[:, None])
            w = np.einsum("ctk,tk->ct", tv, np.cross(e1, d) / det[:, None])
            t = np.einsum("ctk,tk->ct", tv, n / det[:, None])
            inner = np.minimum(np.minimum(u, w), np.minimum(1.0 - u - w, t))
            for f in factors:
                t_max = f * ln
                m = np.minimum(inner, t_max - t)
                tt = t
                if par.any():
                    reach = plane[:, par] <= t_max * PARALLEL + eps
                    m, tt = m.copy(), t.copy()
                    m[:, par] = np.where(reach, 0.0, -np.inf)
                    tt[:, par] = -np.inf  # an ambiguous candidate in front of everything: the closest hit is not robust
                cand = m > -eps
                cut = (m > eps).any(axis=1)
                tc = np.where(cand, tt, np.inf)
                j = np.argmin(tc, axis=1)
                o = out[f]
                o[0][i, a : a + chunk] = cut
                o[1][i, a : a + chunk] = cand.any(axis=1) & ~cut
                o[2][i, a : a + chunk] = tc[rows, j]
                o[3][i, a : a + chunk] = cut & (m[rows, j] > eps)
    return out


# ---- winding number ------------------------------------------------------------------------------------------------
def winding_numbers(verts, points, chunk=1024):
    """Generalized winding number of the soup at each point: sum of the signed solid angles of the triangles / 4 pi"""
    v = np.asarray(verts, np.float64).reshape(-1, 3, 3)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(points))
    for s in range(0, len(points), chunk):
        r = v[None] - points[s : s + chunk, None, None, :]  # (C, T, 3 corners, 3)
        ln = np.linalg.norm(r, axis=3)
        a, b, c = r[:, :, 0], r[:, :, 1], r[:, :, 2]
        num = np.einsum("ctk,ctk->ct", a, np.cross(b, c))
        den = ln.prod(axis=2) + (a * b).sum(2) * ln[:, :, 2] + (b * c).sum(2) * ln[:, :, 0] + (c * a).sum(2) * ln[:, :, 1]
        out[s : s + chunk] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


# ---- triangle against closed unit box ----------------------------------------------------------------------------------
def tri_box_axes(tri):
    """The 13 candidate separating axes of a triangle and an axis-aligned box, normalised: 3 box axes, the triangle's normal,
    9 cross products of a triangle edge with a box axis (those that vanish are dropped)."""
    tri = np.asarray(tri, np.float64)
    edges = np.stack([tri[1] - tri[0], tri[2] - tri[1], tri[0] - tri[2]])
    axes = list(np.eye(3)) + [np.cross(edges[0], edges[1])] + [np.cross(e, x) for e in edges for x in np.eye(3)]
    scale = np.abs(edges).max()
    return np.array([x / np.linalg.norm(x) for x in axes if np.linalg.norm(x) > 1e-12 * scale * scale])


def tri_box_separation(tri, lows):
    """Signed separation of a triangle from the closed unit boxes [low, low + 1]: the largest gap between the two projections
    over the 13 axes.  Negative: they overlap (by the separating-axis theorem); positive: an axis separates them."""
    tri = np.asarray(tri, np.float64)
    ctr = np.asarray(lows, np.float64).reshape(-1, 3) + 0.5
    sep = np.full(len(ctr), -np.inf)
    for ax in tri_box_axes(tri):
        p = tri @ ax
        cc, r = ctr @ ax, 0.5 * np.abs(ax).sum()
        sep = np.maximum(sep, np.maximum(p.min() - (cc + r), (cc - r) - p.max()))
    return sep


def surface_voxels(verts, lo, hi, eps_box=EPS_BOX):
    """Voxels lo <= index < hi (per axis; indices may be negative) that a triangle of the soup overlaps.  Returns (solid, amb),
    arrays of shape hi - lo: solid where some triangle overlaps by more than eps_box or touches EXACTLY (separation 0.0, which
    fp64 yields only where the coordinates involved are integers: the box is closed, and fp32 is exact there too); amb where
    none does but one comes within eps_box."""
    lo, hi = np.asarray(lo, int), np.asarray(hi, int)
    solid, amb = np.zeros(tuple(hi - lo), bool), np.zeros(tuple(hi - lo), bool)
    for tri in _triangles(verts):
        a = np.maximum(np.floor(tri.min(axis=0)).astype(int) - 1, lo)
        b = np.minimum(np.floor(tri.max(axis=0)).astype(int) + 2, hi)
        if np.any(b <= a):
            continue
        idx = np.stack(np.meshgrid(*[np.arange(a[k], b[k]) for k in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
        sep = tri_box_separation(tri, idx)
        i, j, k = (idx - lo).T
        solid[i, j, k] |= (sep < -eps_box) | (sep == 0.0)
        amb[i, j, k] |= (np.abs(sep) <= eps_box) & (sep != 0.0)
    return solid, amb & ~solid


def close_padded(solid, h):
    """The closing of aabb_close.py on the padded grid: max filter then min filter over (2 h + 1)^3 cubes; cells within h of the
    grid's faces are copied through each filter unchanged.  Separable 1-D filters, the out-of-range neighbours neutral."""

    def filt(a, op, neutral):
        out = a
        for ax in range(3):
            p = np.pad(out, [(h, h) if k == ax else (0, 0) for k in range(3)], constant_values=neutral)
            acc = None
            for s in range(2 * h + 1):
                sl = [slice(None)] * 3
                sl[ax] = slice(s, s + a.shape[ax])
                acc = p[tuple(sl)] if acc is None else op(acc, p[tuple(sl)])
            out = acc
        res = a.copy()
        core = tuple(slice(h, n - h) for n in a.shape)
        res[core] = out[core]
        return res

    return filt(filt(solid, np.logical_or, False), np.logical_and, True)


# ---- the four maskers ----------------------------------------------------------------------------------------------
def _shift(a, c, fill=False):
    """b[x] = a[x + c] where x + c is in the box, `fill` elsewhere"""
    out = np.full(a.shape, fill, a.dtype)
    src = tuple(slice(max(s, 0), n + min(s, 0)) for s, n in zip(c, a.shape))
    dst = tuple(slice(max(-s, 0), n + min(-s, 0)) for s, n in zip(c, a.shape))
    out[dst] = a[src]
    return out


class MeshReference:
    """Geometry of one mesh on one grid, computed once: link tables over the cells within `margin` of the mesh's bounding box
    (all 26 directions, length factors 1 and 1.5), winding numbers, surface voxels on the grid padded by 2 * 3.  masks() then
    composes any method / lattice / close_voxels from them."""

    PAD = 6

    def __init__(self, verts, shape, margin=3):
        self.verts = np.asarray(verts, np.float32)
        self.shape = tuple(int(n) for n in shape)
        v = self.verts.astype(np.float64)
        self.lo = np.maximum(np.floor(v.min(axis=0)).astype(int) - margin, 0)
        self.hi = np.minimum(np.floor(v.max(axis=0)).astype(int) + margin, np.array(self.shape) - 1) + 1
        self.window = np.zeros(self.shape, bool)
        self.window[tuple(slice(a, b) for a, b in zip(self.lo, self.hi))] = True
        cells = np.argwhere(self.window)
        hits = link_hits(self.verts, cells + 0.5, DIRS26, (1.0, 1.5))
        self.links = {}
        for f, arrs in hits.items():
            dense = []
            for arr, fill in zip(arrs, (False, False, np.inf, False)):
                full = np.full((26,) + self.shape, fill, arr.dtype)
                full[:, cells[:, 0], cells[:, 1], cells[:, 2]] = arr
                dense.append(full)
            self.links[f] = dense
        wn = np.zeros(self.shape)
        wn[self.window] = winding_numbers(self.verts, cells + 0.5)
        self.winding = wn
        p = self.PAD
        self.vox_solid, self.vox_amb = surface_voxels(self.verts, (-p,) * 3, np.array(self.shape) + p)

    def _dir(self, c):
        return int(np.flatnonzero((DIRS26 == np.asarray(c)).all(axis=1))[0])

    def masks(self, method, c, bc_id, close_voxels=0, with_dist=True):
        """Returns (req, amb, stats): req / amb are dicts with 'bc' (nx, ny, nz) uint8, 'mm' (q, ...) bool and 'dist' (q, ...)
        fp64 (None for AABB or without distances) for masks and distances written into fresh, zero-filled fields; stats
        counts the cut / ambiguous links and solid / ambiguous voxels the case rests on."""
        c = np.asarray(c, int)
        q = c.shape[1]
        cl = [tuple(int(x) for x in c[:, l]) for l in range(q)]
        opp = [cl.index(tuple(-x for x in v)) for v in cl]
        moving = [l for l in range(q) if opp[l] != l]
        shape = self.shape
        bc = np.zeros(shape, np.uint8)
        bc_amb = np.zeros(shape, bool)
        mm, mm_amb = np.zeros((q,) + shape, bool), np.zeros((q,) + shape, bool)
        dist, dist_amb = np.zeros((q,) + shape), np.zeros((q,) + shape, bool)
        stats = dict(cut_links=0, amb_links=0, solid_voxels=0, amb_voxels=0, amb_winding=0)
        p = self.PAD
        crop = tuple(slice(p, p + n) for n in shape)

        if method in ("AABB", "AABB_CLOSE"):
            if method == "AABB":
                S, A = self.vox_solid[crop], self.vox_amb[crop]
                stats.update(solid_voxels=int(S.sum()), amb_voxels=int(A.sum()))
            else:
                h = int(close_voxels)
                off = p - 2 * h
                sub = tuple(slice(off, off + n + 4 * h) for n in shape)
                inner = tuple(slice(2 * h, 2 * h + n) for n in shape)
                empty = close_padded(self.vox_solid[sub], h)[inner]
                full = close_padded((self.vox_solid | self.vox_amb)[sub], h)[inner]
                S, A = empty, full != empty
                stats.update(solid_voxels=int(self.vox_solid[sub].sum()), amb_voxels=int(self.vox_amb[sub].sum()))
            nb_s, nb_a = np.zeros(shape, bool), np.zeros(shape, bool)
            cut, amb, t, t_ok = self.links[1.5]
            for l in moving:
                Sn, An = _shift(S, cl[l]), _shift(A, cl[l])
                nb_s |= Sn
                nb_a |= An
                link = ~S & ~A & Sn & ~An  # certainly a link from a fluid voxel into a solid one
                link_amb = ~S & (An | (A & Sn))
                mm[opp[l]] |= ~S & Sn
                mm_amb[opp[l]] |= link_amb
                if method == "AABB_CLOSE" and with_dist:
                    k = self._dir(cl[l])
                    ln = float(np.sqrt(np.dot(cl[l], cl[l])))
                    hit = np.where(cut[k], (np.where(np.isfinite(t[k]), t[k], 0.0) - 0.5 * ln) / ln, 1.0)
                    dist[l] = np.where(~S & Sn, hit, 0.0)
                    dist_amb[l] = link_amb | (link & (amb[k] | (cut[k] & ~t_ok[k])))
                    stats["cut_links"] += int((link & cut[k]).sum())
                    stats["amb_links"] += int((link & amb[k]).sum())
            bc[:] = np.where(S, BC_SOLID, np.where(nb_s, bc_id, 0))
            bc_amb[:] = ~S & (A | (nb_a & ~nb_s))
        elif method == "RAY":
            cut, amb, t, t_ok = self.links[1.0]
            any_cut, any_amb = np.zeros(shape, bool), np.zeros(shape, bool)
            for l in moving:
                k = self._dir(cl[l])
                ln = float(np.sqrt(np.dot(cl[l], cl[l])))
                mm[opp[l]] |= cut[k]
                mm_amb[opp[l]] |= amb[k]
                any_cut |= cut[k]
                any_amb |= amb[k]
                dist[l] = np.where(cut[k], np.where(np.isfinite(t[k]), t[k], 0.0) / ln, 0.0)
                dist_amb[l] = amb[k] | (cut[k] & ~t_ok[k])
                stats["cut_links"] += int(cut[k].sum())
                stats["amb_links"] += int(amb[k].sum())
            bc[:] = np.where(any_cut, bc_id, 0)
            bc_amb[:] = ~any_cut & any_amb
        elif method == "WINDING":
            S = self.winding > 0.5
            A = np.abs(self.winding - 0.5) <= EPS_WIND
            stats["amb_winding"] = int(A.sum())
            cut, amb, t, t_ok = self.links[1.0]
            tagged, tagged_amb = np.zeros(shape, bool), np.zeros(shape, bool)
            for l in moving:
                k = self._dir(cl[l])
                ln = float(np.sqrt(np.dot(cl[l], cl[l])))
                back = tuple(-x for x in cl[l])  # the solid voxel at x - c_l whose ray along c_l reaches x
                Ss, As = _shift(S, back), _shift(A, back)
                cs, ams = _shift(cut[k], back), _shift(amb[k], back)
                ts, oks = _shift(t[k], back, np.inf), _shift(t_ok[k], back)
                tag = ~S & Ss & cs
                tag_amb = A | As | (~S & Ss & ams)
                mm[l] |= tag
                mm_amb[l] |= tag_amb
                tagged |= tag
                tagged_amb |= tag_amb
                dist[opp[l]] = np.where(tag, (ln - np.where(np.isfinite(ts), ts, 0.0)) / ln, 0.0)
                dist_amb[opp[l]] = tag_amb | (tag & ~oks)
                stats["cut_links"] += int((S & cut[k]).sum())
                stats["amb_links"] += int((S & amb[k]).sum())
            bc[:] = np.where(S, BC_SOLID, np.where(tagged, bc_id, 0))
            bc_amb[:] = A | (~S & ~tagged & tagged_amb)
        else:
            raise ValueError(method)

        # resolve_out_of_bound: a voxel of this id also misses every direction pulled from outside the box
        has_id, idx = bc == bc_id, np.indices(shape)
        for l in moving:
            outside = np.zeros(shape, bool)
            for a in range(3):
                pp = idx[a] - cl[l][a]
                outside |= (pp < 0) | (pp >= shape[a])
            sure = mm[l] & ~mm_amb[l]
            mm_amb[l] = (mm_amb[l] | (bc_amb & outside)) & ~sure & ~(has_id & ~bc_amb & outside)
            mm[l] |= has_id & outside
        if method == "AABB" or not with_dist:
            dist = dist_amb = None
        return dict(bc=bc, mm=mm, dist=dist), dict(bc=bc_amb, mm=mm_amb, dist=dist_amb), stats


def dense_distances(table, q, shape):
    """(q, nx, ny, nz) weights from a HybridBC distance table (cells, (n, q) weights); zero where the table has no row"""
    cells, w = table
    out = np.zeros((q, int(np.prod(shape))), np.float64)
    out[:, np.asarray(cells, np.int64)] = np.asarray(w, np.float64).T
    return out.reshape((q,) + tuple(shape))


def disagreements(req, amb, got_bc, got_mm, got_dist=None, tol=DIST_TOL):
    """Where the code under test leaves what the reference requires: counts of wrong cells outside the ambiguous sets (bc ids,
    missing bits, weights further than tol) and the largest deviation of an unambiguous weight."""
    got_bc = np.asarray(got_bc).reshape(req["bc"].shape)
    got_mm = np.asarray(got_mm).astype(bool)
    out = dict(bc=int(((got_bc != req["bc"]) & ~amb["bc"]).sum()), mm=int(((got_mm != req["mm"]) & ~amb["mm"]).sum()), dist=0, dist_max=0.0)
    if got_dist is not None:
        dev = np.where(amb["dist"], 0.0, np.abs(np.asarray(got_dist, np.float64) - req["dist"]))
        out.update(dist=int((dev > tol).sum()), dist_max=float(dev.max()))
    return out


def check_caps(stats):
    assert stats["amb_links"] <= LINK_CAP * stats["cut_links"], stats
    assert stats["amb_voxels"] <= VOXEL_CAP * stats["solid_voxels"], stats
    assert stats["amb_winding"] == 0, stats


# ---- the mesh zoo ----------------------------------------------------------------------------------------------------
def rotation(axis=(1.0, 2.0**0.5, 3.0**0.5), angle=1.0):
    """A fixed rotation with irrational entries (Rodrigues)"""
    k = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rotated(verts, centre, rot):
    return ((np.asarray(verts, np.float64) - centre) @ rot.T + centre).astype(np.float32)


def box(lo, hi):
    """12 triangles of the axis-aligned box, counter-clockwise seen from outside"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    tris = []
    for ax in range(3):
        u, v = (ax + 1) % 3, (ax + 2) % 3
        for side, at in ((0, lo[ax]), (1, hi[ax])):
            def pt(a, b):
                p = np.empty(3)
                p[ax], p[u], p[v] = at, (lo[u], hi[u])[a], (lo[v], hi[v])[b]
                return p
            quad = [pt(0, 0), pt(1, 0), pt(1, 1), pt(0, 1)]  # counter-clockwise seen from +ax
            if side == 0:
                quad = quad[::-1]
            tris += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.array(tris).reshape(-1, 3).astype(np.float32)


def torus(centre, R, r, nu=24, nv=12, rot=None):
    """nu x nv quads of a torus around the z axis (2 nu nv triangles), outward orientation, optionally rotated about its centre"""
    a = 2 * np.pi * (np.arange(nu + 1) + 0.37) / nu
    b = 2 * np.pi * (np.arange(nv + 1) + 0.21) / nv

    def pt(i, j):
        return np.array([(R + r * np.cos(b[j])) * np.cos(a[i]), (R + r * np.cos(b[j])) * np.sin(a[i]), r * np.sin(b[j])])

    tris = []
    for i in range(nu):
        for j in range(nv):
            p00, p10, p11, p01 = pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)
            tris += [[p00, p10, p11], [p00, p11, p01]]
    v = np.array(tris).reshape(-1, 3)
    if rot is not None:
        v = v @ rot.T
    return (v + np.asarray(centre)).astype(np.float32)


def inward(verts):
    return np.ascontiguousarray(np.asarray(verts).reshape(-1, 3, 3)[:, ::-1].reshape(-1, 3))


def with_zero_area_triangle(verts):
    v = np.asarray(verts).reshape(-1, 3, 3)
    extra = np.stack([v[0, 0], v[0, 1], v[0, 1]])[None]  # two equal corners
    return np.concatenate([v, extra]).reshape(-1, 3).astype(np.float32)
