"""Hand-built scenes for the independent pins (tools/make_independent_golden.py, test_independent.py).

Deterministic numpy (PCG64) clouds in the body frame of the support service (horizontal axis
(0, 0, -1), so a support plane is z = const):

  q4_scene   table (horizontal), then a wall (vertical), then a shelf (horizontal) -- in that
             RANSAC order -- so createNewIdxMap runs with level -1 between two supports and the
             table's -2 tags are overwritten (quirk Q4, supports_segmentation_srv.cpp:145,332)
  q5_scene   a table whose first cloud point is its minimum-x (and minimum-y) point, plus object
             points just inside the true edge: getPointOnPlane's `else if` bbox (Q5, :192-200)
             never lets a running-max point lower xMin, so those objects fall outside
  cluster_cloud  separated blobs of distinct sizes plus sparse clutter, with no point pair within
             1e-6 m of the clustering radius: the cKDTree pin works in float64 and cannot say on
             which side of the float32 radius such a pair falls.  The shell itself (`<` versus `<=`,
             the operation order) is tested in test_neighbourhood_edges.py

and the scenes of test_neighbourhood_edges.py, built so that the neighbourhood kernels' edge paths
decide the result:

  bridged_cells, jittered_radius_lattice, snake   clustering decided by pairs at the radius
  sum_blobs                                        cluster sizes around the sum kernels' block sizes
  pow2_lattice, pow2_plane, clump_and_sheet, far_points   exact ties at the k-th neighbour, more
                                                   candidates than the kNN buffer holds, isolated points

and the scenes of test_primitive_edges.py (these call the oracle to check or to build themselves):

  exact_sphere, exact_cylinder, exact_cone   m low-noise model points whose raw RANSAC inliers are exactly
                                             the labelled points, clutter 1 m away, a model point first and last
  shell_scene                                points placed at the raw model's threshold +- 2e-6 m (two passes)
  octahedron_sphere                          an analytic sphere with probes at the threshold and 1, 2 ulp off it
"""
import math

import numpy as np

from independent import radius2


def _plane_patch(rng, n, x, y, z, noise=0.002):
    p = np.empty((n, 3), np.float64)
    p[:, 0] = rng.uniform(*x, n) if isinstance(x, tuple) else x + rng.normal(0, noise, n)
    p[:, 1] = rng.uniform(*y, n) if isinstance(y, tuple) else y + rng.normal(0, noise, n)
    p[:, 2] = rng.uniform(*z, n) if isinstance(z, tuple) else z + rng.normal(0, noise, n)
    return p


def _box(rng, n, lo, hi):
    return rng.uniform(lo, hi, (n, 3))


def q4_scene(seed=5):
    rng = np.random.default_rng(seed)
    table = _plane_patch(rng, 9000, (0.0, 1.0), (-0.5, 0.5), 0.70)
    wall = _plane_patch(rng, 6000, 1.30, (-0.6, 0.6), (0.0, 1.6))
    shelf = _plane_patch(rng, 3000, (0.2, 0.9), (-0.45, 0.45), 1.25)
    objs = np.concatenate([_box(rng, 500, (0.3, 0.72, 0.0), (0.4, 0.85, 0.1)) @ np.eye(3)[[0, 2, 1]],
                           _box(rng, 400, (0.6, -0.2, 0.72), (0.7, -0.1, 0.85))])
    pts = np.concatenate([table, wall, shelf, objs])
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


def q5_scene(seed=5):
    rng = np.random.default_rng(seed)
    table = _plane_patch(rng, 6000, (0.0, 1.0), (-0.5, 0.5), 0.70, noise=0.001)
    # first table point: the minimum x and minimum y of the table
    table[0] = (-0.01, -0.51, 0.70)
    # objects just inside the true x / y edges (inside x > xmin + 0.02), away from the far edges
    near = _box(rng, 300, (0.015, 0.0, 0.73), (0.04, 0.3, 0.80))
    near_y = _box(rng, 300, (0.3, -0.485, 0.73), (0.6, -0.47, 0.80))
    mid = _box(rng, 500, (0.4, 0.0, 0.73), (0.55, 0.15, 0.85))
    pts = np.concatenate([table, near, near_y, mid]).astype(np.float32)
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


def cluster_cloud(seed, radius=0.03, n_blobs=7):
    """Blobs of distinct sizes (far apart) plus sparse clutter.  One point of every pair whose
    distance lies within 1e-6 of the radius is dropped (removing points changes no other distance)."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    parts = []
    sizes = rng.choice(np.arange(150, 1500, 37), n_blobs, replace=False)
    for b, s in enumerate(sizes):
        c = np.array([0.6 * (b % 4), 0.6 * (b // 4), 1.0 + 0.05 * b])
        parts.append(c + rng.normal(0, 0.025, (s, 3)))
    parts.append(rng.uniform((-0.3, -0.3, 0.5), (2.2, 1.4, 1.8), (400, 3)))
    pts = np.concatenate(parts)
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    t = cKDTree(pts.astype(np.float64))
    shell = t.query_pairs(radius + 1e-6) - t.query_pairs(radius - 1e-6)
    drop = np.zeros(len(pts), bool)
    for i, j in sorted(shell):
        if not (drop[i] or drop[j]):
            drop[j] = True
    pts = pts[~drop]
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


def plain_bbox_on_support(x, y, z, support, idx_map, level, offset=(0.02, 0.02, 0.005), quirk=True):
    """getPointOnPlane (supports_segmentation_srv.cpp:187-238) restated in numpy.  quirk=True is the
    reference's `else if` running bbox (Q5); quirk=False an ordinary min/max bbox, for contrast."""
    sx, sy, sz = (support[:, k].astype(np.float64) for k in range(3))

    def bounds(v):
        if not quirk:
            return float(v.max()), float(v.min())
        prev = np.maximum.accumulate(np.concatenate([[-np.inf], v[:-1]]))
        lows = v[v <= prev]  # not a new running max: the `else if` branch may lower xMin
        return float(v.max()), float(lows.min()) if len(lows) else np.inf

    xmax, xmin = bounds(sx)
    ymax, ymin = bounds(sy)
    off = np.asarray(offset, np.float32).astype(np.float64)
    xmax -= off[0]
    xmin += off[0]
    ymax -= off[1]
    ymin += off[1]
    zmed = math.fsum(sz) / len(sz) + off[2]  # the sequential double sum is exact here (Q10)
    keep = (idx_map != level) & (x > xmin) & (x < xmax) & (z > zmed) & (y > ymin) & (y < ymax)
    return np.stack([x[keep], y[keep], z[keep]], 1)


# ---- neighbourhood edge scenes (test_neighbourhood_edges.py) --------------------------------------
def _split(p):
    p = np.ascontiguousarray(p, np.float32)
    assert len(np.unique(p[np.isfinite(p).all(1)], axis=0)) == np.isfinite(p).all(1).sum(), "duplicate points (A8)"
    return p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()


def bridge_x(xa, side, tol=0.03):
    """The float32 x of bridge point b for a at xa (same y, z): the largest float whose FLANN distance
    to a is still < r^2 ("in"), or the next float up ("out"), by bisection over the float32 bit patterns."""
    r2 = radius2(tol)
    xa = np.float32(xa)

    def linked(bits):
        ex = xa - np.array(bits, np.uint32).view(np.float32)
        return (ex * ex + np.float32(0)) + np.float32(0) < r2

    lo = int(np.float32(xa + np.float32(0.9 * tol)).view(np.uint32))   # linked
    hi = int(np.float32(xa + np.float32(1.1 * tol)).view(np.uint32))   # not linked
    assert linked(lo) and not linked(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if linked(mid) else (lo, mid)
    return np.array(lo if side == "in" else hi, np.uint32).view(np.float32)


def bridge_at(a, tol=0.03):
    """A bridge point b = (a.x + ex, a.y + ey, a.z) whose FLANN distance to a is r^2 exactly: not a
    neighbour under `<`, a neighbour under `<=`.  On x alone no float pair of these cells has it (the
    differences there are even multiples of the radius's ulp and the float radius is odd), so a small
    ey = k 2^-20 is added, the first k from 1000 for which one of the floats around
    a.x + sqrt(r^2 - ey^2) gives (ex ex + ey ey) + 0 == r^2."""
    r2 = radius2(tol)
    for k in range(1000, 10000):
        yb = np.float32(a[1] + np.float32(k * 2.0 ** -20))
        ey = a[1] - yb
        xb = np.float32(float(a[0]) + math.sqrt(float(r2) - float(ey) ** 2))
        for _ in range(4):
            xb = np.nextafter(xb, np.float32(0))
        for _ in range(9):
            ex = a[0] - xb
            if (ex * ex + ey * ey) + np.float32(0) == r2:
                return np.array([xb, yb, a[2]], np.float32)
            xb = np.nextafter(xb, np.float32(1))
    raise AssertionError("no float pair at the radius")


CELL_SIDE = float(np.float32(0.03)) / math.sqrt(3.0) * (1.0 - 1e-4)  # clusters.hip's grid, origin at the minimum


def _bridged_group(rng, na, nb, side, yoff=0.0):
    """(a and b, ball A and ball B) of one bridged cell pair, moved by yoff in y; asserts that ball A
    and a lie in grid cell (2, 2 + yoff / CELL_SIDE, 2) and ball B and b in the cell two over in x (the
    grid's origin is the anchor at 0: cell 2 is [0.03464, 0.05196), cell 4 is [0.06928, 0.08660))."""
    c = np.float32(0.036)
    cy = np.float32(0.036 + yoff)
    ball_a = (np.array([0.036, 0.036 + yoff, 0.036]) + rng.uniform(-0.001, 0.001, (na - 1, 3))).astype(np.float32)
    ball_b = (np.array([0.0855, 0.036 + yoff, 0.036]) + rng.uniform(-0.0008, 0.0008, (nb - 1, 3))).astype(np.float32)
    xa = np.float32(0.0515)
    a = np.array([xa, cy, c], np.float32)
    b = bridge_at(a) if side == "at" else np.array([bridge_x(xa, side), cy, c], np.float32)
    row = 2 + int(round(yoff / CELL_SIDE))
    for pts, cell in ((np.vstack([ball_a, a]), (2, row, 2)), (np.vstack([ball_b, b]), (4, row, 2))):
        assert np.array_equal(np.floor(pts.astype(np.float64) / CELL_SIDE), np.tile(cell, (len(pts), 1))), cell
    return np.stack([a, b]), np.concatenate([ball_a, ball_b])


def bridged_cells(na, nb, side, first, seed=7):
    """An anchor at the origin (it fixes the grid origin: cells of side 0.03 / sqrt(3) (1 - 1e-4) =
    0.017319), ball A (na - 1 points within 0.001 of (0.036, 0.036, 0.036), cell (2, 2, 2)), ball B
    (nb - 1 points within 0.0008 of (0.0855, 0.036, 0.036), cell (4, 2, 2)) and the bridge points
    a = (0.0515, 0.036, 0.036) in A's cell and b = (bridge_x, 0.036, 0.036) in B's (the cells are
    asserted).  The balls are 0.0475 apart and each bridge point is more than 0.033 from the other
    ball, so (a, b) is the only pair that can link the two cells: linked one float below the radius
    ("in"), not linked at the next float ("out"), whose distance is already above r^2, nor exactly at
    r^2 ("at", bridge_at: b up to 0.01 off in y, still in B's cell).  first: a and b carry the lowest
    indices of their cells, else the highest."""
    rng = np.random.default_rng(seed)
    ab, balls = _bridged_group(rng, na, nb, side)
    rest = np.concatenate([np.zeros((1, 3), np.float32), balls])
    rest = rest[rng.permutation(len(rest))]
    return _split(np.concatenate([ab, rest] if first else [rest, ab]))


def bridged_rows(groups=16, na=200, nb=9, seed=37):
    """`groups` bridged cell pairs ("in": each linked by its one pair) eight cells apart in y, one anchor,
    all indices permuted.  Cell A of each pair (na points, more than 64) is the one that probes cell B,
    and a pair's link is seen only when A's points past the first 64 are loaded.  Which slot of its
    cell a point takes is decided by the device's atomics, not by this scene; with the a points at
    random indices, a kernel that never loads past slot 63 finds every link only if all `groups` a
    points sit in the first 64 of their na slots: (64 / 200)^16, about 1e-8, for any order that does
    not know which point is a."""
    rng = np.random.default_rng(seed)
    parts = [np.zeros((1, 3), np.float32)]
    for g in range(groups):
        parts += _bridged_group(rng, na, nb, "in", 8 * g * CELL_SIDE)
    p = np.concatenate(parts)
    return _split(p[rng.permutation(len(p))])


def jittered_radius_lattice(offset=(0.0, 0.0, 0.0), seed=11):
    """A 12^3 lattice at pitch 0.03 with N(0, 0.0015) jitter, permuted (n = 1728): lattice neighbours
    lie on both sides of the clustering radius.  The jitter alone leaves only a handful of pairs
    within 1e-4 relative of r^2 (about 4750 neighbour pairs spread over +-0.002 m), so 240 disjoint
    x-neighbour pairs have their second point moved along the pair's line to a distance of
    r (1 + d), d uniform in +-4e-5: after the rounding to float32 they fall on both sides of r^2,
    the nearest within a few ulp.  offset translates the cloud (in double, before that rounding)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*(np.arange(12) * 0.03,) * 3, indexing="ij"), -1).reshape(-1, 3)
    p = g + rng.normal(0, 0.0015, g.shape)
    r = math.sqrt(float(radius2(0.03)))
    first = np.nonzero((np.arange(len(p)) // 144) % 2 == 0)[0]  # even x layer; its +x neighbour is 144 on
    for i in rng.choice(first, 240, replace=False):
        v = p[i + 144] - p[i]
        p[i + 144] = p[i] + v * (r * (1.0 + rng.uniform(-4e-5, 4e-5)) / np.linalg.norm(v))
    p += np.asarray(offset, np.float64)
    return _split(p[rng.permutation(len(p))])


def snake(n=3000, seed=13):
    """A path of n points with consecutive steps of 0.0299 (chords of a helix of radius 0.3 whose
    turns are 0.05 apart, so only consecutive points are linked), indices shuffled: one component
    strung across thousands of cells."""
    rng = np.random.default_rng(seed)
    rad, c = 0.3, 0.05 / (2 * math.pi)
    lo, hi = 0.0, 0.2  # chord(dt)^2 = (2 rad sin(dt / 2))^2 + (c dt)^2 grows with dt
    for _ in range(100):
        dt = 0.5 * (lo + hi)
        lo, hi = (dt, hi) if (2 * rad * math.sin(dt / 2)) ** 2 + (c * dt) ** 2 < 0.0299 ** 2 else (lo, dt)
    t = np.arange(n) * lo
    p = np.stack([rad * np.cos(t), rad * np.sin(t), c * t], 1)
    return _split(p[rng.permutation(n)])


SUM_BLOB_SIZES = (1, 2, 255, 256, 257, 511, 513)


def sum_blobs(total, seed=17):
    """Tight blobs (offsets within 0.004 of their centres: every pair closer than 0.0139, one clique
    each) 0.25 apart, of SUM_BLOB_SIZES points, plus one with the rest of `total`, all permuted.  The
    last is drawn out into a rod 1.2 m long and 0.008 thick (gaps along it below 0.005, asserted: one
    component): as a tight ball its every point would have the whole ball as radius neighbours, which
    costs a sorted-radius-search restatement of PCL tens of seconds.  The centres lie near x = 0.5,
    y = 100, z = -7, so the three sum chains run at different magnitudes and round on every add.
    Returns x, y, z and the blob of every point."""
    rng = np.random.default_rng(seed)
    sizes = SUM_BLOB_SIZES + (total - sum(SUM_BLOB_SIZES),)
    assert sizes[-1] > max(SUM_BLOB_SIZES)
    parts, blob = [], []
    for b, s in enumerate(sizes):
        centre = np.array([0.5 + 0.25 * b, 100.0 + 0.25 * (b % 3), -7.0 - 0.25 * (b % 2)])
        parts.append(centre + rng.uniform(-0.004, 0.004, (s, 3)))
        blob.append(np.full(s, b))
    parts[-1][:, 0] += rng.uniform(0.0, 1.2, sizes[-1])
    assert np.diff(np.sort(parts[-1][:, 0])).max() < 0.005
    perm = rng.permutation(total)
    return _split(np.concatenate(parts)[perm]) + (np.concatenate(blob)[perm],)


def pow2_lattice(seed=19):
    """12^3 points at pitch 1/64, permuted: every float32 distance is exact, and most queries have
    ties at their k-th distance."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*(np.arange(12) / 64.0,) * 3, indexing="ij"), -1).reshape(-1, 3)
    return _split(g[rng.permutation(len(g))])


def pow2_plane(seed=23):
    """A 40 x 40 planar lattice at pitch 1/128 with z = 0.75, permuted (a grid one cell thick)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(40) / 128.0, np.arange(40) / 128.0, indexing="ij"), -1).reshape(-1, 2)
    p = np.c_[g, np.full(len(g), 0.75)]
    return _split(p[rng.permutation(len(p))])


def clump_and_sheet(seed=29):
    """A 12^3 lattice at pitch 2^-12 centred near (0.5, 0.25, 0.75) inside a sheet of 2500 points
    uniform on [0, 1]^2 with z = 0.75 + N(0, 0.002), permuted; every 97th point's y is NaN (n = 4228).
    Returns x, y, z and a mask of the clump's points."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*((np.arange(12) - 6) / 4096.0,) * 3, indexing="ij"), -1).reshape(-1, 3)
    clump = g + np.array([0.5, 0.25, 0.75])
    sheet = np.c_[rng.uniform(0, 1, (2500, 2)), 0.75 + rng.normal(0, 0.002, 2500)]
    perm = rng.permutation(len(clump) + len(sheet))
    p = np.concatenate([clump, sheet])[perm].astype(np.float32)
    p[::97, 1] = np.nan
    return _split(p) + ((perm < len(clump)),)


def far_points(seed=31):
    """500 random points in a 0.4 m box plus two isolated ones: the ring grows to the whole grid."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.2, 0.2, (500, 3))
    return _split(np.concatenate([p, [[5.0, 5.0, 5.0], [-4.0, 3.0, 9.0]]]))


# ---- primitive edge scenes (test_primitive_edges.py) ----------------------------------------------
def _frame(axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    u = np.cross(a, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    return a, u, np.cross(a, u)


def _unit_rows(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _shuffle_labelled(rng, model, clutter):
    """One shuffle of the model rows and the clutter rows together; then a model row is swapped to index 0
    and another to index n - 1 (the counting and selection kernels' first and last point).  Returns the
    float32 rows and the boolean label of the model rows."""
    m, n = len(model), len(model) + len(clutter)
    perm = rng.permutation(n)
    rows = np.concatenate([model, clutter])[perm]
    label = perm < m
    for end in ((0, n - 1) if m >= 2 else (0,)):
        if not label[end]:
            other = [i for i in np.nonzero(label)[0] if i not in (0, n - 1)][0]
            rows[[end, other]] = rows[[other, end]]
            label[[end, other]] = label[[other, end]]
    return rows.astype(np.float32), label


def _raw_is_label(res, label, what):
    assert res["ok"] and np.array_equal(res["inliers"], np.nonzero(label)[0]), \
        f"{what}: the oracle's raw inliers are not the {int(label.sum())} labelled points"


SPHERE_CENTRE, SPHERE_RADIUS = (0.3, -0.2, 1.1), 0.05
AXIS, CYL_BASE, CYL_RADIUS, CONE_APEX, CONE_HALF_DEG = (0.1, 0.2, 1.0), (0.3, -0.1, 0.9), 0.04, (0.3, -0.1, 1.1), 25.0
CLUTTER_SHIFT = np.array([1.0, 0.0, 0.0])  # the clutter box lies 1 m from the model


def _sphere_points(rng, m, noise):
    d = _unit_rows(rng.normal(size=(m, 3)))
    d[:, 2] = -np.abs(d[:, 2])  # the camera sees one hemisphere
    return np.asarray(SPHERE_CENTRE) + SPHERE_RADIUS * d + rng.normal(0, noise, (m, 3))


def _cylinder_points(rng, m, noise, h=0.15):
    a, u, v = _frame(AXIS)
    t, ph = rng.uniform(0, h, m), rng.uniform(0, 2 * np.pi, m)
    radial = np.cos(ph)[:, None] * u + np.sin(ph)[:, None] * v
    p = np.asarray(CYL_BASE) + t[:, None] * a + CYL_RADIUS * radial + rng.normal(0, noise, (m, 3))
    return np.c_[p, _unit_rows(radial + rng.normal(0, 0.02, (m, 3)))]


def _cone_points(rng, m, noise, h=0.15):
    a, u, v = _frame(AXIS)
    half = np.deg2rad(CONE_HALF_DEG)
    t, ph = rng.uniform(0.03, h, m), rng.uniform(0, 2 * np.pi, m)
    radial = np.cos(ph)[:, None] * u + np.sin(ph)[:, None] * v
    p = np.asarray(CONE_APEX) + t[:, None] * a + (t * np.tan(half))[:, None] * radial + rng.normal(0, noise, (m, 3))
    return np.c_[p, _unit_rows(np.cos(half) * radial - np.sin(half) * a + rng.normal(0, 0.01, (m, 3)))]


def _clutter(rng, n_out, centre, half_side, normals):
    o = np.asarray(centre) + rng.uniform(-half_side, half_side, (n_out, 3))
    return np.c_[o, _unit_rows(rng.normal(size=(n_out, 3)))] if normals else o


def exact_sphere(m, n_out, seed, noise=0.0005, check=True):
    """m points of a sphere (radius 0.05, noise 0.5 mm) and n_out clutter points in a 0.4 m box 1 m away,
    shuffled (_shuffle_labelled).  Returns (P, label); with check, asserts that the sphere service's raw
    RANSAC inliers (the oracle, optimize off) are exactly the labelled points, so its refinement gets
    exactly m residuals."""
    rng = np.random.default_rng(seed)
    P, label = _shuffle_labelled(rng, _sphere_points(rng, m, noise),
                                 _clutter(rng, n_out, SPHERE_CENTRE + CLUTTER_SHIFT, 0.2, False))
    if check:
        import oracle_binding as orc
        _raw_is_label(orc.sphere_segment(*P.T, orc.sphere_params(optimize=False)), label,
                      f"exact_sphere({m}, {n_out}, {seed})")
    return P, label


def exact_cylinder(m, n_out, seed, noise=0.0003, check=True):
    """As exact_sphere for the cylinder service (radius 0.04, noise 0.3 mm, normals within about 0.02 rad of
    the radial direction): (P, N, label)."""
    rng = np.random.default_rng(seed)
    rows, label = _shuffle_labelled(rng, _cylinder_points(rng, m, noise),
                                    _clutter(rng, n_out, CYL_BASE + CLUTTER_SHIFT, 0.2, True))
    P, N = np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3:])
    if check:
        import oracle_binding as orc
        _raw_is_label(orc.cylinder_segment(P, N, orc.cylinder_params(optimize=False)), label,
                      f"exact_cylinder({m}, {n_out}, {seed})")
    return P, N, label


def exact_cone(m, n_out, seed, noise=0.0002, check=True):
    """As exact_sphere for the cone service (half opening angle 25 degrees, 0.03 to 0.15 m from the apex,
    noise 0.2 mm, normals within about 0.01 rad of the surface normal): (P, N, label)."""
    rng = np.random.default_rng(seed)
    rows, label = _shuffle_labelled(rng, _cone_points(rng, m, noise),
                                    _clutter(rng, n_out, CONE_APEX + CLUTTER_SHIFT, 0.2, True))
    P, N = np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3:])
    if check:
        import oracle_binding as orc
        _raw_is_label(orc.cone_segment(P, N, orc.cone_params(optimize=False)), label, f"exact_cone({m}, {n_out}, {seed})")
    return P, N, label


def _far_placeholders(rng, k, normals):
    far = np.array([5.0, 5.0, 5.0]) + rng.uniform(-0.5, 0.5, (k, 3))
    return np.c_[far, _unit_rows(rng.normal(size=(k, 3)))] if normals else far


def shell_scene(model, seed, n_model=3000, n_out=400, n_shell=400, delta=2e-6):
    """A threshold-shell scene in two passes.  Pass 1: n_model model points, n_out clutter points around
    the model and n_shell placeholders metres away, shuffled; the oracle's raw RANSAC (optimize off) gives
    the model M.  Pass 2: the placeholders are overwritten with points whose float64 service distance to M
    is th + d, d uniform in +-delta, half of them inside M's surface and half outside.  For the cylinder
    and the cone their normals are M's surface normal turned by an angle a in [0.2, 0.6] rad, every other
    one reversed (so the fold min(a, pi - a) decides it), and the offset from the surface is solved for
    w a + (1 - w) offset = th + d.  (Normals exactly along M's normal put every placed point where the
    reference's float dot product rounds to 1 - ulp and its acos jumps by 3.5e-4 rad: the oracle then
    differs from the float64 rule by up to 2.3e-7 m, and a band of four times that holds a third of the
    placed points.)  The sampler depends only on (n, seed): the caller asserts that the raw model of the
    final cloud is M again.  Returns (P, N or None, M, the placeholder indices)."""
    import oracle_binding as orc
    rng = np.random.default_rng(seed)
    normals = model != "sphere"
    if model == "sphere":
        pts, centre, seg, prm = _sphere_points(rng, n_model, 0.001), SPHERE_CENTRE, orc.sphere_segment, orc.sphere_params
    elif model == "cylinder":
        pts, centre, seg, prm = _cylinder_points(rng, n_model, 0.001), CYL_BASE, orc.cylinder_segment, orc.cylinder_params
    else:
        # the cone is moved to 0.1 m from the origin: at 1 m the reference's float rounding of a point's foot
        # on the axis (6e-8 m) alone puts it 5.5e-8 m from the float64 rule, and four times that is a band
        # that holds a tenth of the placed points
        pts, centre, seg, prm = _cone_points(rng, n_model, 0.0005), np.array([0.0, 0.0, 0.1]), orc.cone_segment, \
            orc.cone_params
        pts[:, :3] += centre - CONE_APEX
    rows = np.concatenate([pts, _clutter(rng, n_out, centre, 0.2, normals), _far_placeholders(rng, n_shell, normals)])
    perm = rng.permutation(len(rows))
    rows = rows[perm].astype(np.float32)
    shell = np.nonzero(perm >= n_model + n_out)[0]
    P, N = np.ascontiguousarray(rows[:, :3]), (np.ascontiguousarray(rows[:, 3:]) if normals else None)
    p = prm(optimize=False)
    raw = seg(*P.T, p) if model == "sphere" else seg(P, N, p)
    assert raw["ok"]
    M = raw["coef"].astype(np.float64)
    side = np.where(np.arange(n_shell) % 2 == 0, 1.0, -1.0)
    D = p.threshold + rng.uniform(-delta, delta, n_shell)
    if model == "sphere":
        P[shell] = (M[:3] + (M[3] + side * D)[:, None] * _unit_rows(rng.normal(size=(n_shell, 3)))).astype(np.float32)
        return P, None, raw["coef"], shell
    w = p.normal_distance_weight
    u = M[3:6] / np.linalg.norm(M[3:6])
    e = _unit_rows(np.cross(u, rng.normal(size=(n_shell, 3))))  # unit vectors across the axis
    k = (P[raw["inliers"]].astype(np.float64) - M[:3]) @ u   # the inliers' positions along the axis
    k = rng.choice(k, n_shell)
    turn = rng.uniform(0.2, 0.6, n_shell)
    offset = side * (D - w * turn) / (1.0 - w)
    if model == "cylinder":
        rho, surface_n = M[6] + offset, e
    else:
        assert 0.0 < M[6] < np.pi / 2
        rho = np.tan(M[6]) * np.abs(k) + offset
        surface_n = np.sin(M[6]) * (-np.sign(k))[:, None] * u + np.cos(M[6]) * e
    assert (rho > 0).all()
    nrm = np.cos(turn)[:, None] * surface_n + np.sin(turn)[:, None] * np.cross(u, e)  # u x e is across both
    nrm[(np.arange(n_shell) // 2) % 2 == 1] *= -1.0
    P[shell] = (M[:3] + k[:, None] * u + rho[:, None] * e).astype(np.float32)
    N[shell] = nrm.astype(np.float32)
    return P, N, raw["coef"], shell


OCTA_R, OCTA_T = 0.0625, 2.0 ** -7


def octahedron_sphere(k, seed):
    """The six vertices (+-r, 0, 0), (0, +-r, 0), (0, 0, +-r), r = 1/16, k times each, and 60 axis probes at
    |x| = r +- t + j ulp, j = -2 .. 2, t = 2^-7, shuffled.  Every valid 4-sample of the vertices gives the
    sphere (0, 0, 0, r) exactly, coplanar and repeated samples have m11 = 0 and are skipped.  For a probe
    sqrt(x x) = |x| and | |x| - r | = t -+ j ulp are exact in float32, so with threshold t the expected
    inliers follow from the construction: the vertices, the outer probes with j < 0 and the inner ones with
    j > 0; a probe at distance t exactly is out.  Returns (P, expected inlier mask)."""
    rng = np.random.default_rng(seed)
    r, t = np.float32(OCTA_R), np.float32(OCTA_T)
    rows, inl = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            v = np.zeros(3, np.float32)
            v[axis] = sign * r
            rows += [v] * k
            inl += [True] * k
            for shell in (r + t, r - t):
                for j in range(-2, 3):
                    a = np.float32(shell)
                    for _ in range(abs(j)):
                        a = np.nextafter(a, np.float32(1.0 if j > 0 else 0.0))
                    d = np.abs(a - r)  # exact: a and r are multiples of a's ulp, the difference has few bits
                    assert np.float64(d) == abs(np.float64(a) - np.float64(r))
                    v = np.zeros(3, np.float32)
                    v[axis] = sign * a
                    rows.append(v)
                    inl.append(bool(d < t))
    perm = rng.permutation(len(rows))
    return np.stack(rows)[perm], np.array(inl)[perm]
