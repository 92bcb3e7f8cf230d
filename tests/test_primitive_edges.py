"""The sphere, cylinder and cone services at their size and shell edges (sphere.hip, cylinder.hip, cone.hip,
prim_ransac.hpp, compact.hpp, elm.hpp), against references that are not the oracle (tests/independent.py:
sphere_select32 bit-exact; cylinder_distance64 / cone_distance64 through band_check; lm_cost64).  The CPU
tests hold the oracle to those references and check the scenes themselves; the GPU tests hold the HIP path
to the oracle bit for bit (hypotheses, coefficient bits, inlier list; optimize off, then on) and to the same
references, on the same inputs.

A  scenes.exact_{sphere,cylinder,cone}: the raw RANSAC inliers are exactly the m labelled points (asserted),
   so the device Levenberg-Marquardt gets exactly m residuals: m around the lane / unroll boundaries of its
   reductions (m mod 4, mod 8, 64, 72), the 256-thread element loops, stableNorm's 4096 blocks and the last
   LDS-resident workspace (6144 for the sphere, 4096 for cylinder and cone); and m at the refine_kind edges
   (sphere 4 | 5, cylinder and cone 6 | 7, and below).
B  cloud sizes n = m + n_out at the sample size and one above, around the count kernels' block span (2048
   sphere, 1024 cylinder and cone) and around 16384 | 16385 where the selection leaves k_select_small; a
   labelled point sits at index 0 and at index n - 1 and both must come back.
C  scenes.shell_scene: 400 points placed at the raw model's threshold +- 2e-6 m, inside and outside.
D  scenes.octahedron_sphere: an analytic sphere whose model, skipped samples and inliers follow from the
   construction; probes at the threshold exactly (out) and 1 and 2 ulp to either side.
E  max_iterations at the edges of the host replay's chunks (32, 96, 224, 480), on clutter-heavy scenes where
   computeModel runs to the limit, one of them with 30 % duplicated points (skipped samples).

Measured on the CPU with the oracle (the CPU tests print these figures with -s):

  bands   On every scene of A, B, C and E, raw and refined, the oracle's inlier list and the float64 rule
          dist64 < th disagree on no point: the largest |dist64 - th| of a disagreement is 0 for the
          cylinder and 0 for the cone.  4 x 0 is below the floor, so BAND = 1e-7 m for both (the device's
          double acos need not be glibc's in the last bit).  The sphere is compared exactly.
          Two earlier forms of the shell scene C were replaced because they hid the compare: with the
          placed normals exactly along the model's normal the oracle disagreed up to 1.9e-7 m (cylinder)
          and 2.3e-7 m (cone) from the threshold, and with the cone 1 m from the origin up to 5.5e-8 m;
          four times either is a band holding more than 0.5 % of the cloud (see scenes.shell_scene).
  shells  placed points within 10 x BAND = 1e-6 m of the threshold, below | above: cylinder 98 | 95, cone
          100 | 103 (of 400); sphere (exact compare, same reach) 93 | 105.  Inside the band itself: cylinder
          13, cone 18 of 3800 points (0.34 % and 0.47 %); no point of any other scene.
  optimum The oracle's float LM is inside the existing envelopes of its LM_OPTIMUM mode (SPHERE_PCL_ATOL,
          CYL_PCL_TOL, CONE_PCL_TOL) on every scene here, down to m = 5 (sphere) and m = 7 (cylinder, cone),
          so the device is held to them on every scene too.  The largest distances: sphere 6.0e-7 m in a
          coefficient (envelope 5e-6); cylinder 1 - |cos| 6.7e-10, axis distance 1.7e-6 m, radius 4.5e-6 m
          (1e-7, 5e-5, 5e-5); cone 1 - |cos| 1.4e-8, apex 3.2e-5 m, tan^2 6.8e-5 (1e-7, 1e-4, 1e-4), the
          cone's largest at m = 8 and 9.
  seeds   exact_cone(255, 31) with seed 255 missed its exact inlier count (some cone seeds do); seed 2255 is
          used.  Every other exact scene uses seed = m.  The shell scenes use the first seed whose raw model
          survives the overwrite (sphere 1, cylinder 1, cone 2); the octahedron seed 5 (seeds 0, 2, 3, 4 let a
          sample with a probe win).  No scene was replaced because the oracle's refinement raised the cost.
"""
import functools

import numpy as np
import pytest

import independent as ind
import oracle_binding as orc
import scenes
from test_cone import CONE_PCL_TOL, cone_scene, same_cone
from test_cylinder import CYL_PCL_TOL, cylinder_scene, same_line
from test_sphere import SPHERE_PCL_ATOL, sphere_scene

BAND = {"cylinder": 1e-7, "cone": 1e-7}  # metres; see the module docstring


class Model:
    """A service: its oracle restatement, its HIP entry point, its exact scene; first_lm = the fewest inliers
    its refinement runs the Levenberg-Marquardt on (refine_kind 1)."""

    def __init__(self, name, ident, first_lm, segment, params, exact):
        self.name, self.id, self.first_lm = name, ident, first_lm
        self.segment, self.params, self.exact = segment, params, exact

    def oracle(self, P, N, **kw):
        p = self.params(**kw)
        return self.segment(*P.T, p) if N is None else self.segment(P, N, p)

    def gpu(self, ctx, P, N, **kw):
        import torch
        cols = [torch.from_numpy(np.ascontiguousarray(a[:, k])).cuda() for a in (P, N) if a is not None for k in range(3)]
        inl, coef, hyp = getattr(ctx, self.name + "_segment")(*cols, **kw)
        return {"ok": coef is not None, "inliers": inl.cpu().numpy(), "coef": coef, "hypotheses": hyp}

    def threshold(self, **kw):
        return self.params(**kw).threshold

    def distance64(self, P, N, coef):
        w = self.params().normal_distance_weight
        return (ind.cylinder_distance64 if self.name == "cylinder" else ind.cone_distance64)(P, N, coef, w)


MODELS = {
    "sphere": Model("sphere", ind.MODEL_SPHERE, 5, orc.sphere_segment, orc.sphere_params, scenes.exact_sphere),
    "cylinder": Model("cylinder", ind.MODEL_CYLINDER, 7, orc.cylinder_segment, orc.cylinder_params,
                      scenes.exact_cylinder),
    "cone": Model("cone", ind.MODEL_CONE, 7, orc.cone_segment, orc.cone_params, scenes.exact_cone),
}

# ---- the cases -----------------------------------------------------------------------------------
SPHERE_M = [5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 63, 64, 65, 71, 72, 73, 255, 256, 257, 4095, 4096, 4097, 6143, 6144,
            6145, 8192, 8193]
AXIS_M = [7, 8, 9, 11, 12, 13, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
SEEDS = {("cone", 255, 31): 2255}
SHELL_SEEDS = {"sphere": 1, "cylinder": 1, "cone": 2}  # seeds whose raw model survives the overwrite (asserted)


def _lm_case(m):
    return m, (0 if m < 16 else m // 8)


def _size_case(n, sample):
    n_out = 0 if n <= sample + 1 else n // 9
    return n - n_out, n_out


LM_CASES = ([("sphere",) + _lm_case(m) for m in [4] + SPHERE_M] +
            [(name,) + _lm_case(m) for name in ("cylinder", "cone") for m in [6] + AXIS_M])
SIZE_CASES = ([("sphere",) + _size_case(n, 4) for n in (4, 5, 2047, 2048, 2049, 16383, 16384, 16385)] +
              [("cylinder",) + _size_case(n, 2) for n in (2, 3, 1023, 1024, 1025, 16383, 16384, 16385)] +
              [("cone",) + _size_case(n, 3) for n in (3, 4, 1023, 1024, 1025, 16383, 16384, 16385)])
EXACT_CASES = list(dict.fromkeys(LM_CASES + SIZE_CASES))
ITERATION_LIMITS = (0, 1, 31, 32, 33, 95, 96, 97, 223, 224, 225, 479, 480, 481)


def _id(case):
    return "-".join(str(c) for c in case)


@functools.lru_cache(maxsize=None)
def exact_case(name, m, n_out):
    """(P, N, label, oracle raw, oracle refined) of an exact scene, computed once per session."""
    md = MODELS[name]
    out = md.exact(m, n_out, SEEDS.get((name, m, n_out), m))
    P, N, label = (out[0], None, out[1]) if name == "sphere" else out
    for a in (P, N, label):
        if a is not None:
            a.setflags(write=False)
    return P, N, label, md.oracle(P, N, optimize=False), md.oracle(P, N)


@functools.lru_cache(maxsize=None)
def shell_case(name):
    md = MODELS[name]
    P, N, M, shell = scenes.shell_scene(name, SHELL_SEEDS[name])
    return P, N, M, shell, md.oracle(P, N, optimize=False), md.oracle(P, N)


@functools.lru_cache(maxsize=None)
def limit_scene(kind):
    """Clutter-heavy scenes on which computeModel's k stays above every limit tested."""
    if kind == "sphere":
        return sphere_scene(300, 1500, 41), None
    if kind == "sphere_dup":  # 540 of 1800 points are copies of six clutter points: samples with m11 == 0
        P = sphere_scene(300, 1500, 42)
        rng = np.random.default_rng(42)
        d = np.linalg.norm(P.astype(np.float64) - (0.3, -0.2, 1.1), axis=1)
        src = rng.choice(np.nonzero(d > 0.1)[0], 6, replace=False)
        dup = rng.choice(np.setdiff1d(np.arange(len(P)), src), 540, replace=False)
        P[dup] = P[src[np.arange(540) % 6]]
        return P, None
    if kind == "cylinder":
        return cylinder_scene(100, 1900, 43)[:2]
    return cone_scene(100, 1900, 44)[:2]


LIMIT_KINDS = {"sphere": "sphere", "sphere_dup": "sphere", "cylinder": "cylinder", "cone": "cone"}


@functools.lru_cache(maxsize=None)
def limit_case(kind, max_iterations):
    P, N = limit_scene(kind)
    return MODELS[LIMIT_KINDS[kind]].oracle(P, N, optimize=False, max_iterations=max_iterations)


# ---- the checks shared by the oracle (CPU) and the HIP path (GPU) -------------------------------------
def check_selection(md, P, N, res, **kw):
    """The inlier list of `res` against the independent reference at res's own coefficients: exactly for the
    sphere, by the band rule for cylinder and cone.  Returns how many points lie inside the band."""
    th = md.threshold(**kw)
    prm = md.params()
    lo, hi = (prm.min_angle, prm.max_angle) if md.name == "cone" else (prm.radius_min, prm.radius_max)
    if not lo <= float(res["coef"][-1]) <= hi:  # isModelValid (the limits): selectWithinDistance returns nothing
        assert len(res["inliers"]) == 0
        return 0
    if md.name == "sphere":
        assert np.array_equal(res["inliers"], ind.sphere_select32(P, res["coef"], th))
        return 0
    missing, extra, in_band = ind.band_check(md.distance64(P, N, res["coef"]), th, res["inliers"], BAND[md.name])
    assert len(missing) == 0 and len(extra) == 0, (missing, extra)
    assert in_band <= 0.005 * len(P), f"{in_band} of {len(P)} points inside the band: the scene hides the compare"
    return in_band


def check_refinement(md, P, raw, ref):
    """The refined model against the starting model over the pre-refinement inliers: the float64 cost does
    not rise where the Levenberg-Marquardt ran; below that the model is kept (sphere: bit for bit; cylinder
    and cone: everything but the direction, which is only normalised)."""
    m = len(raw["inliers"])
    if m >= md.first_lm:
        before = ind.lm_cost64(md.id, P, raw["inliers"], raw["coef"])
        after = ind.lm_cost64(md.id, P, raw["inliers"], ref["coef"])
        assert after <= before, (m, before, after)
        return before, after
    if md.name == "sphere":
        assert np.array_equal(ref["coef"].view(np.int32), raw["coef"].view(np.int32))
    else:
        assert np.array_equal(ref["coef"][[0, 1, 2, 6]].view(np.int32), raw["coef"][[0, 1, 2, 6]].view(np.int32))
        d = raw["coef"][3:6].astype(np.float64)
        # the raw direction already has unit float length (1 +- 1.2e-7); dividing it again moves a component
        # by that plus one rounding (6e-8)
        assert np.allclose(ref["coef"][3:6], d / np.linalg.norm(d), rtol=0, atol=3e-7)
    return None


def envelope(md, a, b):
    """(inside the model's existing PCL-LM envelope, the distances) of coefficients a against the optimum b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if md.name == "sphere":
        d = float(np.max(np.abs(a - b)))
        return d < SPHERE_PCL_ATOL, (d,)
    d1, d2 = a[3:6] / np.linalg.norm(a[3:6]), b[3:6] / np.linalg.norm(b[3:6])
    ang = 1 - abs(float(d1 @ d2))
    if md.name == "cylinder":
        dist = (ang, float(np.linalg.norm(np.cross(d1, b[:3] - a[:3]))), abs(abs(a[6]) - abs(b[6])))
        return same_line(a, b, **CYL_PCL_TOL), dist
    b6 = b[6] if d1 @ d2 > 0 else np.pi - b[6]
    dist = (ang, float(np.linalg.norm(a[:3] - b[:3])), abs(np.tan(a[6]) ** 2 - np.tan(b6) ** 2))
    return same_cone(a, b, **CONE_PCL_TOL), dist


def optimum(md, P, N):
    with orc.lm_mode(orc.LM_OPTIMUM):
        return md.oracle(P, N)


@functools.lru_cache(maxsize=None)
def exact_optimum(name, m, n_out):
    P, N = exact_case(name, m, n_out)[:2]
    return optimum(MODELS[name], P, N)["coef"]


@functools.lru_cache(maxsize=None)
def shell_optimum(name):
    P, N = shell_case(name)[:2]
    return optimum(MODELS[name], P, N)["coef"]


def same_result(got, want):
    """The HIP result is the oracle's: hypotheses, coefficient bits, inlier list."""
    assert got["hypotheses"] == want["hypotheses"]
    assert got["ok"] == want["ok"]
    if want["ok"]:
        assert np.array_equal(got["coef"].view(np.int32), want["coef"].view(np.int32)), (got["coef"], want["coef"])
        assert np.array_equal(got["inliers"], want["inliers"])
    else:
        assert len(got["inliers"]) == 0


def shell_population(md, P, N, M, shell, th):
    """(below, above): the placed points within 10 bands (sphere: 1e-6 m) under and over the threshold."""
    if md.name == "sphere":
        d = np.abs(np.linalg.norm(P[shell].astype(np.float64) - M[:3].astype(np.float64), axis=1) - float(M[3]))
        reach = 1e-6
    else:
        d = md.distance64(P[shell], N[shell], M)
        reach = 10 * BAND[md.name]
    return int(((d < th) & (d > th - reach)).sum()), int(((d >= th) & (d < th + reach)).sum())


# ---- A, B: exact inlier counts and cloud sizes --------------------------------------------------------
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_oracle_exact_scene(case):
    name, m, n_out = case
    md = MODELS[name]
    P, N, label, raw, ref = exact_case(*case)
    assert len(P) == m + n_out and label.sum() == m
    assert raw["ok"] and np.array_equal(raw["inliers"], np.nonzero(label)[0])  # the LM gets exactly m residuals
    assert label[0] and (label[-1] or m < 2) and raw["inliers"][0] == 0 and raw["inliers"][-1] == len(P) - 1
    assert ref["ok"] and ref["hypotheses"] == raw["hypotheses"]
    band = [check_selection(md, P, N, r) for r in (raw, ref)]
    cost = check_refinement(md, P, raw, ref)
    inside, dist = envelope(md, ref["coef"], exact_optimum(*case))
    print(f"{_id(case)}: hypotheses {raw['hypotheses']}, in band {band}, cost {cost}, to optimum {dist} inside {inside}")
    assert inside, dist


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXACT_CASES, ids=_id)
def test_hip_exact_scene(ctx, case):
    name, m, n_out = case
    md = MODELS[name]
    P, N, label, raw, ref = exact_case(*case)
    got_raw = md.gpu(ctx, P, N, optimize=False)
    same_result(got_raw, raw)
    assert got_raw["inliers"][0] == 0 and got_raw["inliers"][-1] == len(P) - 1  # the first and the last point
    check_selection(md, P, N, got_raw)
    got = md.gpu(ctx, P, N)
    same_result(got, ref)
    check_selection(md, P, N, got)
    check_refinement(md, P, got_raw, got)
    inside, dist = envelope(md, got["coef"], exact_optimum(*case))
    assert inside, dist


# ---- C: the threshold shell ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_oracle_shell(name):
    md = MODELS[name]
    P, N, M, shell, raw, ref = shell_case(name)
    assert np.array_equal(raw["coef"].view(np.int32), M.view(np.int32))  # the overwrite left the raw model alone
    below, above = shell_population(md, P, N, M, shell, md.threshold())
    listed = np.isin(shell, raw["inliers"])
    print(f"{name}: {below} | {above} placed points within 10 bands below | above the threshold, "
          f"{listed.sum()} of {len(shell)} placed points are inliers")
    assert below >= 20 and above >= 20
    assert 100 <= listed.sum() <= 300  # the placed points fall on both sides
    band = [check_selection(md, P, N, r) for r in (raw, ref)]
    print(f"{name}: in band {band}, cost {check_refinement(md, P, raw, ref)}")
    inside, dist = envelope(md, ref["coef"], shell_optimum(name))
    assert inside, dist


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_hip_shell(ctx, name):
    md = MODELS[name]
    P, N, M, shell, raw, ref = shell_case(name)
    got_raw = md.gpu(ctx, P, N, optimize=False)
    same_result(got_raw, raw)
    check_selection(md, P, N, got_raw)
    got = md.gpu(ctx, P, N)
    same_result(got, ref)
    check_selection(md, P, N, got)
    check_refinement(md, P, got_raw, got)
    inside, dist = envelope(md, got["coef"], shell_optimum(name))
    assert inside, dist


# ---- D: the analytic sphere ---------------------------------------------------------------------------
OCTA = dict(k=50, seed=5)


def check_octahedron(res, want):
    assert res["ok"]
    assert np.array_equal(res["coef"] + np.float32(0), np.array([0, 0, 0, scenes.OCTA_R], np.float32))  # -0 + 0 = +0
    assert np.array_equal(res["inliers"], np.nonzero(want)[0])


def test_oracle_octahedron_sphere():
    P, want = scenes.octahedron_sphere(**OCTA)
    assert want.sum() == 6 * OCTA["k"] + 24 and len(P) == 6 * OCTA["k"] + 60
    res = orc.sphere_segment(*P.T, orc.sphere_params(threshold=scenes.OCTA_T, optimize=False))
    check_octahedron(res, want)
    assert np.array_equal(res["inliers"], ind.sphere_select32(P, res["coef"], scenes.OCTA_T))
    # the samples on the way (getSamples replayed on std::mt19937's outputs): some were skipped (m11 == 0)
    draws, sh, used, skipped = orc.mt19937(12345, 4 * 200), np.arange(len(P)), 0, 0
    for a in range(200):
        for i in range(4):
            j = i + int(draws[4 * a + i] >> 1) % (len(P) - i)
            sh[i], sh[j] = sh[j], sh[i]
        ok = orc.sphere_from4(P[sh[:4]])[0]
        used, skipped = used + ok, skipped + (not ok)
        if used == res["hypotheses"]:
            break
    print(f"octahedron: {res['hypotheses']} hypotheses, {skipped} samples skipped")
    assert used == res["hypotheses"] == len(res["counts"]) and skipped >= 1


@pytest.mark.gpu
def test_hip_octahedron_sphere(ctx):
    P, want = scenes.octahedron_sphere(**OCTA)
    want_res = orc.sphere_segment(*P.T, orc.sphere_params(threshold=scenes.OCTA_T, optimize=False))
    got = MODELS["sphere"].gpu(ctx, P, None, threshold=scenes.OCTA_T, optimize=False)
    check_octahedron(got, want)
    same_result(got, want_res)


# ---- E: the iteration limit at the replay's chunk edges -----------------------------------------------
@pytest.mark.parametrize("kind", list(LIMIT_KINDS))
def test_oracle_iteration_limits(kind):
    got = [limit_case(kind, it)["hypotheses"] for it in ITERATION_LIMITS]
    assert got == [0] + [it + 1 for it in ITERATION_LIMITS[1:]], got  # computeModel stops at the limit, never earlier
    assert not limit_case(kind, 0)["ok"]
    P, N = limit_scene(kind)
    for it in ITERATION_LIMITS[1:]:
        check_selection(MODELS[LIMIT_KINDS[kind]], P, N, limit_case(kind, it))
    if kind == "sphere_dup":
        assert len(P) - len(np.unique(P, axis=0)) == 540


@pytest.mark.gpu
@pytest.mark.parametrize("max_iterations", ITERATION_LIMITS)
@pytest.mark.parametrize("kind", list(LIMIT_KINDS))
def test_hip_iteration_limits(ctx, kind, max_iterations):
    P, N = limit_scene(kind)
    md = MODELS[LIMIT_KINDS[kind]]
    want = limit_case(kind, max_iterations)
    got = md.gpu(ctx, P, N, optimize=False, max_iterations=max_iterations)
    same_result(got, want)
    if want["ok"]:
        check_selection(md, P, N, got)
