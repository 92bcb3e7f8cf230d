"""The two neighbourhood kernels at their edges, against brute-force references (tests/independent.py:
radius_components, brute_knn, seq_sum32 -- dense O(n^2) numpy float32 in FLANN's operation order, no
search structure shared with the oracle).  CPU tests hold the oracle to them; GPU tests hold the HIP
path to the same expectations and to the oracle bit for bit.

A  Euclidean clustering (clusters.hip, k_cell_union) where single point pairs at the radius decide
   the components: two cells whose only link is one pair one float below, above or exactly at the
   radius, at cell populations around the kernel's 64-point loads and 8-pair groups
   (scenes.bridged_cells); a jittered
   lattice with hundreds of pairs at the radius, also at negative and at large coordinates; a 3000-point
   chain across thousands of cells; sixteen 200-point cells each linked to its neighbour by one pair
   (scenes.bridged_rows: the loads past a cell's first 64 points must find it, whatever slot it took).
B  Cluster sums at the switch between k_sums and the exact-sum walk (16384 members) and at clusters
   around its 256-element segments (scenes.sum_blobs).
C  k nearest neighbours (normals.hip, k_knn / nn_select): exact ties at the k-th distance (power-of-two
   lattices), more candidates in one ring than the 1024-slot buffer holds (scenes.clump_and_sheet),
   isolated points, k from 1 to 64, and the covariance accumulation order on the sheet.
"""
import ctypes
import functools

import numpy as np
import pytest

import independent as ind
import oracle_binding as orc
import scenes

TOL = 0.03
POPULATIONS = [(1, 1), (7, 7), (64, 64), (65, 65), (129, 71), (200, 9)]
BRIDGED = [(na, nb, side, first) for na, nb in POPULATIONS for side in ("in", "out", "at") for first in (True, False)]
CLOUDS = {
    "lattice": lambda: scenes.jittered_radius_lattice(),
    "lattice_negative": lambda: scenes.jittered_radius_lattice((-3.2, -3.1, -3.3)),
    "lattice_1000m": lambda: scenes.jittered_radius_lattice((1000.0, 1000.0, 1000.0)),
    "snake": lambda: scenes.snake(),
    "bridged_rows": lambda: scenes.bridged_rows(),
}


def _tuples(members):
    return [tuple(int(i) for i in m) for m in members]


def _oracle_clusters(x, y, z, min_size=0, max_size=None):
    n = len(x)
    return orc.euclidean_clusters(x, y, z, TOL, min_rate=min_size / n, max_rate=(max_size or n) / n, min_input_size=0)


@functools.lru_cache(maxsize=None)
def cluster_case(key):
    """(cloud, brute-force components, oracle clusters) of a scene, computed once per session."""
    xyz = scenes.bridged_cells(*key) if isinstance(key, tuple) else CLOUDS[key]()
    return xyz, ind.radius_components(*xyz, TOL)[1], _oracle_clusters(*xyz)


def check_members(members, comps):
    """The clusters (all sizes kept) are the brute-force components, largest first, members ascending."""
    members = _tuples(members)
    assert sorted(members) == sorted(comps)
    assert all(len(a) >= len(b) for a, b in zip(members, members[1:]))
    assert all(all(i < j for i, j in zip(m, m[1:])) for m in members)


def near_radius_pairs(x, y, z, rel=1e-4):
    """(pairs below, pairs at or above) r^2 within a relative rel of it."""
    dd = ind.pair_dd32(x, y, z, np.arange(len(x)))[np.triu_indices(len(x), 1)].astype(np.float64)
    r2 = float(ind.radius2(TOL))
    return int(((dd < r2) & (dd > r2 * (1 - rel))).sum()), int(((dd >= r2) & (dd < r2 * (1 + rel))).sum())


def lattice_size_bounds(comps):
    """min_size / max_size that components of the lattice actually have (both bounds inclusive)."""
    sizes = sorted({len(c) for c in comps})
    assert len(sizes) >= 4
    return sizes[1], sizes[-2]


# ---- A: clusters, oracle ------------------------------------------------------------------------
def test_bridge_is_one_float_wide():
    """The "in" and "out" bridge positions are adjacent floats with the FLANN distance of (a, b) below r^2
    at the first and not at the second; the "at" bridge's distance is r^2 exactly (only `<` versus `<=`
    tells it from a neighbour)."""
    xa, r2 = np.float32(0.0515), ind.radius2(TOL)
    xin, xout = scenes.bridge_x(xa, "in"), scenes.bridge_x(xa, "out")
    assert np.nextafter(xin, np.float32(1)) == xout
    assert (xa - xin) * (xa - xin) < r2 <= (xa - xout) * (xa - xout)
    x, y, z = scenes.bridged_cells(1, 1, "at", True)  # a, b, anchor
    assert ind.pair_dd32(x, y, z, np.array([0]))[0, 1] == r2
    print(f"r^2 {r2!r}: in {(xa - xin) * (xa - xin)!r}, out {(xa - xout) * (xa - xout)!r}, at b = {x[1]!r}, {y[1]!r}")


@pytest.mark.parametrize("na,nb,side,first", BRIDGED)
def test_oracle_bridged_cells(na, nb, side, first):
    (x, y, z), comps, cl = cluster_case((na, nb, side, first))
    # the anchor alone and, linked by (a, b) only, the two cells together or apart
    assert sorted(len(c) for c in comps) == ([1, na + nb] if side == "in" else sorted([1, na, nb]))
    check_members([c["inliers"] for c in cl], comps)


@pytest.mark.parametrize("name", list(CLOUDS))
def test_oracle_clusters_vs_brute_force(name):
    (x, y, z), comps, cl = cluster_case(name)
    check_members([c["inliers"] for c in cl], comps)
    if name == "lattice":
        below, above = near_radius_pairs(x, y, z)
        print(f"lattice: {len(comps)} components, {below} pairs below and {above} above r^2 within 1e-4")
        assert below >= 50 and above >= 50 and len(comps) > 10
    if name == "lattice_negative":
        assert min(x.min(), y.min(), z.min()) < -3.0
    if name == "snake":
        assert len(comps) == 1 and len(comps[0]) == 3000
    if name == "bridged_rows":  # the anchor and 16 linked cell pairs
        assert sorted(len(c) for c in comps) == [1] + [209] * 16


def test_oracle_lattice_size_bounds():
    (x, y, z), comps, _ = cluster_case("lattice")
    lo, hi = lattice_size_bounds(comps)
    cl = _oracle_clusters(x, y, z, lo, hi)
    kept = [c for c in comps if lo <= len(c) <= hi]
    assert {len(c) for c in kept} >= {lo, hi} and len(kept) < len(comps)
    assert sorted(_tuples(c["inliers"] for c in cl)) == sorted(kept)


# ---- B: cluster sums, oracle --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sums_case(total):
    x, y, z, blob = scenes.sum_blobs(total)
    return (x, y, z), blob, _oracle_clusters(x, y, z)


def expected_sums(x, y, z, members):
    return np.array([ind.seq_sum32(v[members]) for v in (x, y, z)], np.float32)


@pytest.mark.parametrize("total", [16383, 16384])
def test_oracle_sum_blobs(total):
    """The oracle's clusters are the generator's blobs, and its centroid is the sequential float32 sum
    over the ascending members divided by n + 1 (Q7).  The inputs notice another summation order: every
    blob of 255 or more members sums to other bits when its members are added in reverse."""
    (x, y, z), blob, cl = sums_case(total)
    sizes = [len(c["inliers"]) for c in cl]
    assert sum(sizes) == total and sorted(sizes) == sorted(scenes.SUM_BLOB_SIZES + (total - sum(scenes.SUM_BLOB_SIZES),))
    for c in cl:
        m = c["inliers"]
        assert np.array_equal(m, np.nonzero(blob == blob[m[0]])[0])
        s = expected_sums(x, y, z, m)
        assert np.array_equal(s / np.float32(len(m) + 1), c["centroid"])
        if len(m) >= 255:
            assert not np.array_equal(s, expected_sums(x, y, z, m[::-1])), len(m)


# ---- C: k nearest neighbours, oracle ------------------------------------------------------------
KNN_CLOUDS = {
    "pow2_lattice": (lambda: scenes.pow2_lattice(), (3, 7, 50, 63, 64)),
    "pow2_plane": (lambda: scenes.pow2_plane(), (3, 7, 50, 63, 64)),
    "clump_and_sheet": (lambda: scenes.clump_and_sheet()[:3], (50, 64)),
    "far_points": (lambda: scenes.far_points(), (50,)),
}
KNN_CASES = [(name, k) for name, (_, ks) in KNN_CLOUDS.items() for k in ks]
# The covariance pin on the sheet queries of clump_and_sheet at k = 50: the oracle's own error against
# covariance32 + float64 eigh, measured on this scene on the CPU (test_oracle_sheet_covariance prints
# them), and the bounds at 8x (room for a differently rounded but correct eigen-solve).
ORACLE_SINE_MAX, ORACLE_CURV_MAX = 1.375e-7, 1.247e-7
SINE_BOUND, CURV_BOUND = 8 * ORACLE_SINE_MAX, 8 * ORACLE_CURV_MAX


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """(cloud, brute-force lists for k = 64): the list for a smaller k is its prefix."""
    xyz = KNN_CLOUDS[name][0]()
    return xyz, ind.brute_knn(*xyz, 64)


@functools.lru_cache(maxsize=None)
def clump_mask():
    return scenes.clump_and_sheet()[3]


def check_lists(nn, cnt, brute, k):
    """Every query's list and count equal the brute-force ones (all queries)."""
    for q, b in enumerate(brute):
        assert cnt[q] == len(b[:k]) and np.array_equal(nn[q, :cnt[q]], b[:k]), q


def check_nan_queries(x, y, z, nrm, cur, cnt):
    bad = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
    assert np.all(np.isnan(nrm[bad])) and np.all(np.isnan(cur[bad])) and np.all(cnt[bad] == 0)


def tie_share(x, y, z, brute, k):
    """Share of queries whose k-th and (k+1)-th brute-force neighbours are at the same float distance."""
    def d(q, j):
        ex, ey, ez = x[q] - x[j], y[q] - y[j], z[q] - z[j]
        return (ex * ex + ey * ey) + ez * ez
    return np.mean([d(q, b[k - 1]) == d(q, b[k]) for q, b in enumerate(brute) if len(b) > k])


@pytest.mark.parametrize("name,k", KNN_CASES)
def test_oracle_knn_vs_brute_force(name, k):
    (x, y, z), brute = knn_case(name)
    nrm, cur, (nn, cnt) = orc.normal_estimation(x, y, z, k, neighbours=True)
    check_lists(nn, cnt, brute, k)
    check_nan_queries(x, y, z, nrm, cur, cnt)
    if name.startswith("pow2") and k == 50:
        assert tie_share(x, y, z, brute, k) > 0.5  # most queries cut a tie at the k-th distance by index


def test_clump_overflows_the_candidate_buffer():
    """normals.hip's grid: pilot cells of extent / 64 (0.0156 here), rescaled by sqrt(16 / points per
    occupied pilot cell).  The sheet has about one point per occupied pilot cell and the clump sits in
    one or two, so that ratio is about 2 and the final cell about 0.045 -- in any case not below 0.8 x
    extent / 64 unless occupied cells held more than 25 points on average, which 2500 sheet points
    spread over 64 x 64 cells rule out.  The clump's side (0.0027) is far below one cell, so ring 1 (3^3
    cells) of every clump query holds the whole clump: more than 1100 candidates at exactly tied
    distances in one ring pass, against a 1024-slot buffer pruned when 960 are in.  The in-flight prune
    (nn_select mid-ring) must run and must cut ties by index."""
    x, y, z, clump = scenes.clump_and_sheet()
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    assert len(x) == 4228 and (~fin).sum() == 44
    extent = max(float(v[fin].max() - v[fin].min()) for v in (x, y, z))
    inside = clump & fin
    side = max(float(v[inside].max() - v[inside].min()) for v in (x, y, z))
    assert inside.sum() >= 1100 and side < 0.8 * extent / 64
    # sheet points per occupied pilot cell: far below 25
    sheet = fin & ~clump
    pilot = np.floor(np.stack([x[sheet] - x[fin].min(), y[sheet] - y[fin].min()], 1) / (extent / 64))
    assert sheet.sum() / len(np.unique(pilot, axis=0)) < 4


def sheet_errors(x, y, z, clump, brute, nrm, cur, k=50):
    """Over the sheet's finite queries: (max sine of the angle between the normal and the float64
    eigenvector of covariance32 over the brute-force list, max curvature error against |w0 / trace|,
    share of queries skipped because (w1 - w0) < 0.05 w2)."""
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    sheet = np.nonzero(fin & ~clump)[0]
    sine = curv = 0.0
    skipped = 0
    for q in sheet:
        c = ind.covariance32(x, y, z, brute[q][:k])[0].astype(np.float64)
        w, v = np.linalg.eigh(c)
        if (w[1] - w[0]) < 0.05 * w[2]:
            skipped += 1
            continue
        sine = max(sine, float(np.linalg.norm(np.cross(v[:, 0], nrm[q].astype(np.float64)))))
        curv = max(curv, abs(abs(w[0] / np.trace(c)) - float(cur[q])))
    return sine, curv, skipped / len(sheet)


def check_sheet(nrm, cur, who):
    """Measured for the oracle on this scene: sine 1.375e-7, curvature 1.247e-7, 1 of 2471 sheet queries
    skipped (0.04 %).  Bounds (8x): sine 1.1e-6, curvature 9.98e-7; at most 5 % skipped."""
    (x, y, z), brute = knn_case("clump_and_sheet")
    sine, curv, skipped = sheet_errors(x, y, z, clump_mask(), brute, nrm, cur)
    print(f"{who}: sheet normals sine max {sine:.4g} (bound {SINE_BOUND:.4g}), curvature max error {curv:.4g} "
          f"(bound {CURV_BOUND:.4g}), skipped {skipped:.4%}")
    assert skipped <= 0.05
    assert sine <= SINE_BOUND and curv <= CURV_BOUND
    return sine, curv


def test_oracle_sheet_covariance():
    (x, y, z), _ = knn_case("clump_and_sheet")
    nrm, cur = orc.normal_estimation(x, y, z, 50)
    check_sheet(nrm, cur, "oracle")  # prints the figures the bounds rest on


@pytest.mark.parametrize("k", [1, 2])
def test_oracle_knn_below_three(k):
    (x, y, z), _ = knn_case("clump_and_sheet")
    nrm, cur, (_, cnt) = orc.normal_estimation(x, y, z, k, neighbours=True)
    assert np.all(cnt == 0) and np.all(np.isnan(nrm)) and np.all(np.isnan(cur))


# ---- the HIP path against the same expectations ----------------------------------------------------
def _hip_clusters(ctx, x, y, z, min_size=1, max_size=10 ** 9):
    return ctx.euclidean_clusters(x, y, z, TOL, min_size, max_size)


def _hip_clusters_dev(ctx, x, y, z, min_size=1, max_size=10 ** 9):
    import torch
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, y, z)]
    return [(i.cpu().numpy(), s) for i, s in ctx.euclidean_clusters_dev(*d, TOL, min_size, max_size)]


def _hip_clusters_aos(ctx, x, y, z, stride, min_size=1, max_size=10 ** 9):
    from pitt_object_table_segmentation_amd import _lib as L
    from pitt_object_table_segmentation_amd.api import _host_copy
    from test_aos_gpu import _aos, _fp
    a = _aos(x, y, z, stride)
    out = L.ClusterList()
    rc = L.lib.pitt_euclidean_clusters_aos(ctx.h, _fp(a), len(x), stride, TOL, min_size, max_size, ctypes.byref(out))
    assert rc == 0
    cl = [out.clusters[i] for i in range(out.n_clusters)]
    return [(_host_copy(c.indices, (c.size,), np.int32), np.array(list(c.sum_xyz), np.float32)) for c in cl]


def check_hip_clusters(ctx, key, entries=False):
    (x, y, z), comps, ref = cluster_case(key)
    dev = _hip_clusters(ctx, x, y, z)
    check_members([c.indices for c in dev], comps)
    assert _tuples(c.indices for c in dev) == _tuples(c["inliers"] for c in ref)  # the oracle's order too
    if entries:
        others = [_hip_clusters_dev(ctx, x, y, z), _hip_clusters_aos(ctx, x, y, z, 12), _hip_clusters_aos(ctx, x, y, z, 16)]
        for got in others:
            assert _tuples(i for i, _ in got) == _tuples(c.indices for c in dev)
            assert all(np.array_equal(s, c.sum_xyz) for (_, s), c in zip(got, dev))


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb,side,first", BRIDGED)
def test_hip_bridged_cells(ctx, na, nb, side, first):
    check_hip_clusters(ctx, (na, nb, side, first), entries=(na, nb) == (129, 71))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CLOUDS))
def test_hip_clusters_vs_brute_force(ctx, name):
    check_hip_clusters(ctx, name, entries=name == "lattice")


@pytest.mark.gpu
def test_hip_lattice_size_bounds(ctx):
    (x, y, z), comps, _ = cluster_case("lattice")
    lo, hi = lattice_size_bounds(comps)
    kept = sorted(c for c in comps if lo <= len(c) <= hi)
    ref = _tuples(c["inliers"] for c in _oracle_clusters(x, y, z, lo, hi))
    got = _tuples(c.indices for c in _hip_clusters(ctx, x, y, z, lo, hi))
    assert sorted(got) == kept and got == ref
    for got in (_hip_clusters_dev(ctx, x, y, z, lo, hi), _hip_clusters_aos(ctx, x, y, z, 12, lo, hi),
                _hip_clusters_aos(ctx, x, y, z, 16, lo, hi)):
        assert _tuples(i for i, _ in got) == ref


@pytest.mark.gpu
@pytest.mark.parametrize("total", [16383, 16384])
def test_hip_sum_blobs(ctx, total):
    """One member short of the exact-sum walk (k_sums) and at its first size, with clusters of 255, 256,
    257, 511 and 513 members around the walk's 256-element segments: every sum_xyz is the sequential
    float32 sum over the ascending members, bit for bit."""
    (x, y, z), _, ref = sums_case(total)
    dev = _hip_clusters(ctx, x, y, z)
    assert _tuples(c.indices for c in dev) == _tuples(c["inliers"] for c in ref)
    assert sum(len(c.indices) for c in dev) == total
    for c, r in zip(dev, ref):
        assert np.array_equal(c.sum_xyz, expected_sums(x, y, z, c.indices)), len(c.indices)
        assert np.array_equal(c.sum_xyz / np.float32(len(c.indices) + 1), r["centroid"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", KNN_CASES)
def test_hip_knn_vs_brute_force(ctx, name, k):
    from test_normals import _check, _gpu
    (x, y, z), brute = knn_case(name)
    nrm, cur, nn, cnt = _gpu(ctx, x, y, z, k)
    check_lists(nn, cnt, brute, k)
    check_nan_queries(x, y, z, nrm, cur, cnt)
    _check(ctx, x, y, z, k)  # lists, normals and curvature equal the oracle's bit for bit
    if (name, k) == ("clump_and_sheet", 50):
        check_sheet(nrm, cur, "hip")


@pytest.mark.gpu
def test_hip_knn_k_limits(ctx):
    import torch
    from pitt_object_table_segmentation_amd import _lib as L
    from pitt_object_table_segmentation_amd.api import PittError
    from test_normals import _check
    (x, y, z), _ = knn_case("clump_and_sheet")
    for k in (1, 2):  # fewer than 3 neighbours: counts 0, NaN normals, as the oracle
        _check(ctx, x, y, z, k)
    d = [torch.from_numpy(a).cuda() for a in (x, y, z)]
    for k in (0, 65):
        with pytest.raises(PittError) as e:
            ctx.normal_estimation(*d, k=k)
        assert e.value.code == L.PITT_E_INVALID
