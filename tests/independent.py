"""Independent restatements used to pin the oracle from outside (TEST INFRASTRUCTURE ONLY).

Nothing here calls the oracle: numpy float32 restatements of PCL 1.7's plane distance test and
covariance, float64 eigen-solves, and scipy graph components for Euclidean clustering.

  select(x, y, z, c)          SampleConsensusModelPlane::selectWithinDistance / countWithinDistance
                              (sac_model_plane.hpp): |c . (p, 1)| < th with the 4-lane dot summed in
                              SSE2 predux order (c0 x + c2 z) + (c1 y + c3) (A3), float32, th as double
  covariance32(...)           computeMeanAndCovarianceMatrix (centroid.hpp): nine float accumulators,
                              sequential in inlier order (np.cumsum is sequential), accu *= 1/n (A9)
  plane_expectations(...)     eig64 / lsq64 planes and their tolerances (tools/make_independent_golden.py)
  cluster_labels(...)         cKDTree.query_pairs + connected_components, clusterize's size filter
  radius_components(...)      the radius graph by the dense float32 distance matrix in FLANN's operation
                              order ((ex ex + ey ey) + ez ez < r^2), connected_components
  brute_knn(...)              exhaustive k nearest neighbours ordered by (float32 distance, index)
  seq_sum32(v)                one sequential float32 sum
  sphere_select32(P, c, t)    SampleConsensusModelSphere::selectWithinDistance in numpy float32, bit-exact:
                              |sqrt((dx dx + dy dy) + dz dz) - r| < float32(t)
  cylinder_distance64(...)    SampleConsensusModelCylinder / Cone::getDistancesToModel in plain float64 (the
  cone_distance64(...)        distance to the surface and the folded normal angle, weighted); not the float
                              operation order, so results are compared through band_check
  band_check(d, th, inl, b)   the points an inlier list must have (d < th - b) and must not have (d > th + b)
  lm_residuals64(model, P)    the OptimizationFunctor residuals of the three primitives in float64
  lm_cost64(model, P, inl, c) their sum of squares over an inlier list
"""
import numpy as np

TH = 0.007
MODEL_SPHERE, MODEL_CYLINDER, MODEL_CONE = 0, 1, 2


def select(x, y, z, c, th=TH):
    c = np.asarray(c, np.float32)
    d = (c[0] * x + c[2] * z) + (c[1] * y + c[3])  # float32 throughout, no FMA in numpy
    return np.nonzero(np.abs(d).astype(np.float64) < th)[0].astype(np.int32)


def covariance32(x, y, z, idx):
    X, Y, Z = x[idx], y[idx], z[idx]
    acc = np.array([np.cumsum(v, dtype=np.float32)[-1] for v in (X * X, X * Y, X * Z, Y * Y, Y * Z, Z * Z, X, Y, Z)],
                   np.float32)
    acc = acc * (np.float32(1) / np.float32(len(idx)))
    mx, my, mz = acc[6], acc[7], acc[8]
    c = np.empty((3, 3), np.float32)
    c[0, 0], c[0, 1], c[0, 2] = acc[0] - mx * mx, acc[1] - mx * my, acc[2] - mx * mz
    c[1, 1], c[1, 2], c[2, 2] = acc[3] - my * my, acc[4] - my * mz, acc[5] - mz * mz
    c[1, 0], c[2, 0], c[2, 1] = c[0, 1], c[0, 2], c[1, 2]
    return c, np.array([mx, my, mz], np.float64)


def covariance64(x, y, z, idx):
    p = np.stack([x[idx], y[idx], z[idx]], 1).astype(np.float64)
    m = p.mean(0)
    return (p - m).T @ (p - m) / len(idx), m


def _plane(cov, centroid):
    w, v = np.linalg.eigh(np.asarray(cov, np.float64))
    n = v[:, 0]
    return np.r_[n, -n @ centroid], w


def plane_distance(a, b):
    """Max abs difference of two planes after scaling both to a unit normal and aligning signs."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a / np.linalg.norm(a[:3]), b / np.linalg.norm(b[:3])
    return float(np.abs(a - np.sign(a[:3] @ b[:3]) * b).max())


def plane_expectations(x, y, z, best_coef):
    idx = select(x, y, z, best_coef)
    out = {"best_count": np.array([len(idx)])}
    if len(idx) < 4:  # optimizeModelCoefficients keeps the hypothesis
        c = np.asarray(best_coef, np.float64)
        out.update(eig64=c, lsq64=c, tol_eig=np.array([1e-6]), tol_lsq=np.array([1e-6]))
        return out
    c32, m32 = covariance32(x, y, z, idx)
    c64, m64 = covariance64(x, y, z, idx)
    eig, w = _plane(c32, m32)
    lsq, _ = _plane(c64, m64)
    gap = max(w[1] - w[0], 1e-30)
    scale = 1.0 + float(np.abs(m32).max())  # d = -n . centroid carries the normal's error
    # PCL's eigen33 clamps the smallest root to 0 (computeRoots2) when the scaled determinant is
    # below FLT_EPSILON or the float covariance came out indefinite; otherwise it solves the cubic
    s32 = c32.astype(np.float64) / max(float(np.abs(c32).max()), 1e-30)
    clamped = w[0] <= 0 or abs(np.linalg.det(s32)) < np.finfo(np.float32).eps
    tol_eig = (1e-5 + (2.0 * abs(w[0]) / gap if clamped else 0.0)) * scale
    dc = np.linalg.norm(c32.astype(np.float64) - c64, 2)
    tol_lsq = tol_eig + 2.0 * dc / gap * scale
    out.update(eig64=eig, lsq64=lsq, tol_eig=np.array([tol_eig]), tol_lsq=np.array([tol_lsq]))
    return out


def cluster_labels(x, y, z, radius=0.03, min_rate=0.01, max_rate=0.99):
    """Components of the radius graph, kept when round(n min_rate) <= size <= round(n max_rate),
    labelled 0.. by decreasing size; -1 for points in no kept cluster."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    p = np.stack([x, y, z], 1).astype(np.float64)
    n = len(p)
    pairs = cKDTree(p).query_pairs(radius, output_type="ndarray")
    g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    sizes = np.bincount(comp)
    lo, hi = int(np.floor(n * min_rate + 0.5)), int(np.floor(n * max_rate + 0.5))
    kept = [c for c in np.argsort(-sizes, kind="stable") if lo <= sizes[c] <= hi]
    if len({int(sizes[c]) for c in kept}) != len(kept):
        raise ValueError("cluster sizes must be distinct for an order-independent fixture")
    lab = np.full(n, -1, np.int32)
    for rank, c in enumerate(kept):
        lab[comp == c] = rank
    return lab


def radius2(tol):
    """KdTreeFLANN::radiusSearch's squared radius: (float)((double)(float)tol * (float)tol)."""
    return np.float32(np.float64(np.float32(tol)) ** 2)


def pair_dd32(x, y, z, rows):
    """FLANN L2_Simple between points `rows` and every point: (ex ex + ey ey) + ez ez in float32."""
    ex, ey, ez = (v[rows, None] - v[None, :] for v in (x, y, z))
    return (ex * ex + ey * ey) + ez * ez


def radius_components(x, y, z, tol, block=512):
    """Components of the graph with an edge where the float32 FLANN distance is < radius2(tol), by the
    dense O(n^2) distance matrix (n up to about 6000); a point with a non-finite coordinate is a
    singleton.  Returns (per-point component label, the components as ascending index tuples)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    x, y, z = (np.ascontiguousarray(v, np.float32) for v in (x, y, z))
    n, r2 = len(x), radius2(tol)
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    ii, jj = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, n, block):
            rows = np.arange(b, min(b + block, n))
            i, j = np.nonzero((pair_dd32(x, y, z, rows) < r2) & fin[rows, None] & fin[None, :])
            ii.append(i + b)
            jj.append(j)
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    g = coo_matrix((np.ones(len(ii), np.int8), (ii, jj)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    order = np.argsort(lab, kind="stable")
    cuts = np.nonzero(np.diff(lab[order]))[0] + 1
    return lab, [tuple(int(i) for i in c) for c in np.split(order, cuts)]


def brute_knn(x, y, z, k):
    """Per finite query its k nearest finite points (itself included, fewer when there are fewer),
    ordered by (float32 FLANN distance of d = q - p, index); a non-finite query gets an empty list."""
    x, y, z = (np.ascontiguousarray(v, np.float32) for v in (x, y, z))
    fin = np.nonzero(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))[0]
    fx, fy, fz = x[fin], y[fin], z[fin]
    out = [np.zeros(0, np.int64)] * len(x)
    for q in fin:
        dx, dy, dz = x[q] - fx, y[q] - fy, z[q] - fz
        d = (dx * dx + dy * dy) + dz * dz
        out[q] = fin[np.lexsort((fin, d))[:k]]
    return out


def seq_sum32(v):
    """The sequential float32 chain ((v0 + v1) + v2) + ... (np.cumsum does not reassociate)."""
    return np.cumsum(np.asarray(v, np.float32), dtype=np.float32)[-1]


def labels_from_clusters(n, clusters):
    lab = np.full(n, -1, np.int32)
    for rank, idx in enumerate(clusters):
        lab[np.asarray(idx)] = rank
    return lab


# ---- the primitive services (test_primitive_edges.py) ----------------------------------------------
def sphere_select32(P, coef, t):
    """sac_model_sphere.hpp selectWithinDistance in float32: the centre subtracted per axis, the three
    squares summed left to right, sqrt, minus the radius, abs, compared with the float threshold."""
    P = np.asarray(P, np.float32)
    c = np.asarray(coef, np.float32)
    dx, dy, dz = P[:, 0] - c[0], P[:, 1] - c[1], P[:, 2] - c[2]
    with np.errstate(invalid="ignore"):
        d = np.abs(np.sqrt((dx * dx + dy * dy) + dz * dz) - c[3])
        return np.nonzero(d < np.float32(t))[0].astype(np.int32)


def _unit64(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _folded_angle64(a, b):
    """The angle between unit vectors, folded to [0, pi / 2] (getAngle3D, then min(a, pi - a))."""
    ang = np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0))
    return np.minimum(ang, np.pi - ang)


def _axis_frame64(P, N, coef):
    """A point's foot on the axis line (coef[:3], coef[3:6]), its distance to the line, the unit radial
    direction and its unit normal, all float64."""
    c = np.asarray(coef, np.float64)
    p, n = np.asarray(P, np.float64), np.asarray(N, np.float64)
    u = c[3:6] / np.linalg.norm(c[3:6])
    v = p - c[:3]
    foot = c[:3] + (v @ u)[:, None] * u
    rad = p - foot
    return c, foot, np.linalg.norm(rad, axis=1), _unit64(rad), _unit64(n)


def cylinder_distance64(P, N, coef, w):
    """|w a + (1 - w) | |p - axis| - r | |: a the folded angle between the point's normal and the radial
    direction (sac_model_cylinder.hpp getDistancesToModel)."""
    c, _, dist, radial, n = _axis_frame64(P, N, coef)
    return np.abs(w * _folded_angle64(n, radial) + (1.0 - w) * np.abs(dist - c[6]))


def cone_distance64(P, N, coef, w):
    """|w a + (1 - w) | |p - axis| - tan(angle) |apex - foot| | |: a the folded angle between the point's
    normal and the cone's normal sin(angle) h + cos(angle) radial at the point's height, h the unit vector
    from the foot to the apex (sac_model_cone.hpp getDistancesToModel)."""
    c, foot, dist, radial, n = _axis_frame64(P, N, coef)
    h = c[:3] - foot
    hn = np.linalg.norm(h, axis=1)
    cone_n = np.sin(c[6]) * _unit64(h) + np.cos(c[6]) * radial
    return np.abs(w * _folded_angle64(n, _unit64(cone_n)) + (1.0 - w) * np.abs(dist - np.tan(c[6]) * hn))


def band_check(dist64, th, inliers, band):
    """(missing, extra, in_band): the points with dist64 < th - band that the inlier list lacks, the listed
    points with dist64 > th + band, and how many points lie inside the band (they may go either way).  A
    non-finite distance never counts as an inlier."""
    d = np.asarray(dist64, np.float64)
    listed = np.zeros(len(d), bool)
    listed[np.asarray(inliers, np.int64)] = True
    with np.errstate(invalid="ignore"):
        must, must_not = d < th - band, ~(d <= th + band)
    return np.nonzero(must & ~listed)[0], np.nonzero(must_not & listed)[0], int((~must & ~must_not).sum())


def lm_residuals64(model, P):
    """The OptimizationFunctor residuals of sac_model_{sphere,cylinder,cone}.h as a function of the
    coefficients, over the points P, in float64 (the operation order of the oracle's double LM)."""
    px, py, pz = (P[:, k].astype(np.float64) for k in range(3))

    def f(q):
        if model == MODEL_SPHERE:
            dx, dy, dz = px - q[0], py - q[1], pz - q[2]
            return np.sqrt((dx * dx + dy * dy) + dz * dz) - q[3]
        su = (q[3] * q[3] + q[4] * q[4]) + q[5] * q[5]
        vx, vy, vz = q[0] - px, q[1] - py, q[2] - pz
        wx, wy, wz = q[4] * vz - q[5] * vy, q[5] * vx - q[3] * vz, q[3] * vy - q[4] * vx
        d2 = ((wx * wx + wy * wy) + wz * wz) / su
        if model == MODEL_CYLINDER:
            return d2 - q[6] * q[6]
        k = (((px - q[0]) * q[3] + (py - q[1]) * q[4]) + (pz - q[2]) * q[5]) / su
        hx, hy, hz = k * q[3], k * q[4], k * q[5]
        r = np.tan(q[6]) * np.sqrt((hx * hx + hy * hy) + hz * hz)
        return d2 - r * r
    return f


def lm_cost64(model, P, inliers, coef):
    """The float64 sum of squared residuals of `coef` over the points listed in `inliers`."""
    r = lm_residuals64(model, np.asarray(P)[np.asarray(inliers, np.int64)])(np.asarray(coef, np.float64))
    return float((r * r).sum())
