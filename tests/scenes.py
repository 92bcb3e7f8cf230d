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
