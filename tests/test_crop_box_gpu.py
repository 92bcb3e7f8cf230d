"""The device CropBox arm filter (pitt_crop_boxes, pitt_srv_arm_filter) against a numpy float32
restatement of PCL 1.7's CropBox<PointXYZ>::applyFilter applied n_boxes times in a row, as the arm
filter service does (arm_filter_srv.cpp:66-103, :134-140).  Element-wise float32 ufuncs round every
operation and never fuse, which is the stated order; the restatement reads pitt_crop_box fields, so it
never depends on the library's own matrix builder.  Kept coordinates, the kept count and the per-box
removed counts are compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import oracle_binding as orc
import pitt_object_table_segmentation_amd as pitt
from pitt_object_table_segmentation_amd import _lib as L

pytestmark = pytest.mark.gpu

# arm_filter_srv.cpp:32-35
FOREARM = ((-0.040, -0.120, -0.190), (0.340, 0.120, 0.105))
ELBOW = ((-0.090, -0.135, -0.160), (0.440, 0.135, 0.110))


def ref_crop(x, y, z, boxes, negative, dense):
    """The five stage steps of pitt_crop_boxes (include/pitt_seg.h) in float32: (keep mask, removed[k])."""
    f = np.float32
    n = len(x)
    alive = np.ones(n, bool)
    removed = np.zeros(len(boxes), np.int64)
    if not dense and len(boxes):
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        removed[0] += int((~fin).sum())
        alive &= fin
    with np.errstate(invalid="ignore", over="ignore"):
        for k, b in enumerate(boxes):
            lx, ly, lz = x, y, z
            if b.has_translation:
                lx, ly, lz = lx - f(b.translation[0]), ly - f(b.translation[1]), lz - f(b.translation[2])
            if b.has_rotation:
                r = [f(v) for v in b.inv_rotation]
                lx, ly, lz = ((r[0] * lx + r[1] * ly) + r[2] * lz, (r[3] * lx + r[4] * ly) + r[5] * lz,
                              (r[6] * lx + r[7] * ly) + r[8] * lz)
                assert lx.dtype == np.float32
            outside = ((lx < f(b.min[0])) | (ly < f(b.min[1])) | (lz < f(b.min[2])) |
                       (lx > f(b.max[0])) | (ly > f(b.max[1])) | (lz > f(b.max[2])))
            ok = outside if negative else ~outside
            removed[k] += int((alive & ~ok).sum())
            alive &= ok
    return alive, removed


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in arrays]


def _bits(planes):
    return np.stack([p.cpu().numpy() for p in planes], 1).view(np.uint32)


def _check(ctx, x, y, z, boxes, negative, dense, dev=None):
    keep, removed = ref_crop(x, y, z, boxes, negative, dense)
    out, rem = ctx.crop_boxes(*(dev or _dev(x, y, z)), boxes, negative=negative, dense=dense)
    want = np.stack([x[keep], y[keep], z[keep]], 1).view(np.uint32)
    assert out[0].numel() == int(keep.sum())
    assert np.array_equal(rem, removed)
    assert np.array_equal(_bits(out), want)
    return keep, removed


def _raw_box(mn, mx, translation=(0, 0, 0), rot=None):
    b = L.CropBox()
    b.min[:], b.max[:], b.translation[:] = [list(map(float, v)) for v in (mn, mx, translation)]
    b.has_translation = int(any(np.float32(t) != 0 for t in translation))
    b.inv_rotation[:] = [float(v) for v in (np.eye(3) if rot is None else np.asarray(rot)).reshape(9)]
    b.has_rotation = 0 if rot is None else 1
    return b


# ---- sizes ---------------------------------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 16383, 16384, 16385, 3 * 16384 + 77]
SEED = 15  # chosen on the restatement alone: with 2047 points every box removes some and some are kept


def _arm_boxes():
    """The four default boxes at four distinct random poses around the cube's centre."""
    rng = np.random.default_rng(SEED)
    boxes = []
    for mn, mx in (FOREARM, FOREARM, ELBOW, ELBOW):
        boxes.append(pitt.crop_box(mn, mx, translation=rng.uniform(-0.12, 0.12, 3), rpy=rng.uniform(-0.5, 0.5, 3)))
    return boxes


def _cube(n):
    """Uniform in [-0.6, 0.6]^3; a smaller cloud is a prefix of a larger one."""
    p = np.random.default_rng(SEED + 1).uniform(-0.6, 0.6, (3, SIZES[-1])).astype(np.float32)
    return p[0, :n].copy(), p[1, :n].copy(), p[2, :n].copy()


@pytest.mark.parametrize("negative", [1, 0])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n, negative):
    """Slice (64), tile (2048) and super-tile (16,384) edges, and more than one scan entry."""
    boxes = _arm_boxes()
    assert all(b.has_rotation and b.has_translation for b in boxes)
    x, y, z = _cube(n)
    keep, removed = ref_crop(x, y, z, boxes, negative, True)
    if n >= 2047:
        assert (removed > 0).all() and keep.sum() > 0, (removed, keep.sum())
    _check(ctx, x, y, z, boxes, negative, True)


@pytest.mark.parametrize("negative", [1, 0])
def test_all_kept_and_all_removed(ctx, negative):
    x, y, z = _cube(16385)
    far = pitt.crop_box(*FOREARM, translation=(5.0, 5.0, 5.0), rpy=(0.3, -0.2, 0.1))
    cover = pitt.crop_box((-2, -2, -2), (2, 2, 2), rpy=(0.1, 0.2, 0.3))  # the cube's corners stay inside
    for box, all_inside in ((far, False), (cover, True)):
        keep, removed = _check(ctx, x, y, z, [box], negative, True)
        assert keep.all() == (all_inside != bool(negative)) and keep.any() == keep.all()
        assert removed[0] == (0 if keep.all() else 16385)


# ---- faces ---------------------------------------------------------------------------------------
def test_faces_are_inside(ctx):
    mn, mx = (-0.25, -0.5, -0.125), (0.5, 0.25, 0.375)
    box = pitt.crop_box(mn, mx)
    assert not box.has_rotation and not box.has_translation
    pts, kind = [], []
    for c in range(3):
        for face, outward in ((np.float32(mn[c]), -np.inf), (np.float32(mx[c]), np.inf)):
            for k, v in (("face", face), ("outer", np.nextafter(face, np.float32(outward))),
                         ("inner", np.nextafter(face, np.float32(-outward)))):
                p = np.zeros(3, np.float32)  # the origin is inside the box
                p[c] = v
                pts.append(p)
                kind.append(k)
    x, y, z = np.array(pts, np.float32).T.copy()
    keep, removed = _check(ctx, x, y, z, [box], 1, True)
    assert [bool(k) for k in keep] == [k == "outer" for k in kind]   # negative: faces are removed with the inside
    keep, _ = _check(ctx, x, y, z, [box], 0, True)
    assert [bool(k) for k in keep] == [k != "outer" for k in kind]


# ---- arithmetic order ------------------------------------------------------------------------------
def test_rotation_is_evaluated_left_to_right_without_fma(ctx):
    """Points placed within a few ulps of a face of a box under a random non-orthonormal matrix: a fused
    or re-associated row evaluation moves many of them across the face."""
    rng = np.random.default_rng(31)
    f = np.float32
    m = 20000
    for row in range(3):
        r = rng.uniform(0.3, 1.5, (3, 3)) * rng.choice([-1.0, 1.0], (3, 3))
        r32 = r.astype(np.float32)
        mn, mx = [-100.0] * 3, [100.0] * 3
        mn[row], mx[row] = -0.5, 0.7
        box = _raw_box(mn, mx, rot=r32)
        x, y = rng.normal(scale=3.0, size=(2, m)).astype(np.float32)
        face = np.where(np.arange(m) % 2 == 0, f(mn[row]), f(mx[row])).astype(np.float64)
        rr = r32[row].astype(np.float64)
        z = ((face - (rr[0] * x + rr[1] * y)) / rr[2]).astype(np.float32)
        z = (z.view(np.int32) + rng.integers(-2, 3, m).astype(np.int32)).view(np.float32)  # +-2 ulps
        # the restatement itself tells the two associations apart on these points
        a = (r32[row, 0] * x + r32[row, 1] * y) + r32[row, 2] * z
        b = r32[row, 0] * x + (r32[row, 1] * y + r32[row, 2] * z)
        flips = int(((a < f(mn[row])) != (b < f(mn[row]))).sum() + ((a > f(mx[row])) != (b > f(mx[row]))).sum())
        assert flips > 100, flips
        dev = _dev(x, y, z)
        for negative in (1, 0):
            keep, _ = _check(ctx, x, y, z, [box], negative, True, dev)
            assert 0.1 * m < keep.sum() < 0.9 * m
    # four such boxes in a chain, with translations, coordinates of scale 3
    boxes = [_raw_box(rng.uniform(-3, -1, 3), rng.uniform(1, 3, 3), rng.normal(size=3),
                      rng.normal(size=(3, 3)).astype(np.float32)) for _ in range(4)]
    x, y, z = rng.normal(scale=3.0, size=(3, 100003)).astype(np.float32)
    for negative in (1, 0):
        _check(ctx, x, y, z, boxes, negative, True)


# ---- non-finite points -----------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("negative", [0, 1])
def test_non_finite_points(ctx, dense, negative):
    rng = np.random.default_rng(17)
    n = 2049 + 300
    p = rng.uniform(-0.6, 0.6, (3, n)).astype(np.float32)
    specials = [np.nan, np.inf, -np.inf, -0.0]
    i = 0
    for c in range(3):            # one special value in one coordinate ...
        for s in specials:
            for _ in range(8):
                p[c, 5 + 7 * i] = s
                i += 1
    for s in specials:            # ... and in all three
        p[:, 5 + 7 * i] = s
        i += 1
    x, y, z = p
    rotated = [pitt.crop_box(*FOREARM, translation=(0.05, -0.02, 0.1), rpy=(0.3, -0.4, 0.2)),
               pitt.crop_box(*ELBOW, translation=(-0.1, 0.05, -0.05), rpy=(-0.2, 0.1, 0.5))]
    plain = [pitt.crop_box(*FOREARM), pitt.crop_box(*ELBOW, translation=(0.1, 0.0, -0.1))]
    # a zero entry in the matrix: inf * 0 = NaN ("inside") with dense, dropped at stage 0 without
    axis = [pitt.crop_box((-0.3, -0.3, -0.3), (0.3, 0.3, 0.3), rpy=(0.0, 0.0, 0.7))]
    for boxes in (rotated, plain, axis, rotated + plain, []):  # no box: a copy, non-finite points included
        _check(ctx, x, y, z, boxes, negative, dense)


# ---- misaligned planes -----------------------------------------------------------------------------
def test_misaligned_planes(ctx):
    boxes = _arm_boxes()
    x, y, z = _cube(16385)
    dx, dy, dz = _dev(x, y, z)
    _check(ctx, x[1:], y[1:], z[1:], boxes, 1, True, dev=(dx[1:], dy[1:], dz[1:]))
    _check(ctx, x[3:], y[1:-2], z[2:-1], boxes, 1, True, dev=(dx[3:], dy[1:-2], dz[2:-1]))


# ---- arguments -------------------------------------------------------------------------------------
def test_arguments(ctx):
    x, y, z = _cube(5000)
    dev = _dev(x, y, z)
    out, rem = ctx.crop_boxes(*dev, [])                       # no box: a copy
    assert len(rem) == 0 and np.array_equal(_bits(out), np.stack([x, y, z], 1).view(np.uint32))
    eight = _arm_boxes() + [pitt.crop_box(*ELBOW, translation=(0.3 * k - 0.4, 0.2, -0.3), rpy=(0.1 * k, 0.2, 0.3))
                            for k in range(4)]
    _check(ctx, x, y, z, eight, 1, True, dev)
    with pytest.raises(pitt.PittError) as e:
        ctx.crop_boxes(*dev, eight + eight[:1])
    assert e.value.code == L.PITT_E_INVALID
    arr = (L.CropBox * 4)(*_arm_boxes())
    o = [torch.empty(5000, dtype=torch.float32, device="cuda") for _ in range(3)]
    m = ctypes.c_int64()
    ptr = [t.data_ptr() for t in dev]
    lib = L.lib
    assert lib.pitt_crop_boxes(ctx.h, *ptr, 5000, arr, 4, 1, 1, ptr[0], o[1].data_ptr(), o[2].data_ptr(),
                               ctypes.byref(m), None) == L.PITT_E_INVALID          # ox == x
    assert lib.pitt_crop_boxes(ctx.h, *ptr, 5000, arr, 4, 1, 1, o[0].data_ptr(), None, o[2].data_ptr(),
                               ctypes.byref(m), None) == L.PITT_E_INVALID          # a null output
    assert lib.pitt_crop_boxes(ctx.h, *ptr, 5000, arr, -1, 1, 1, *(t.data_ptr() for t in o), ctypes.byref(m),
                               None) == L.PITT_E_INVALID
    assert np.array_equal(dev[0].cpu().numpy(), x)            # the rejected calls touched nothing
    _check(ctx, x, y, z, list(arr), 1, True, dev)             # the context is still usable


def test_kernels_are_profiled(ctx):
    x, y, z = _cube(16385)
    dev = _dev(x, y, z)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        out, _ = ctx.crop_boxes(*dev, _arm_boxes())
        kept = out[0].numel()
        mask = 8 * 32 * -(-16385 // 2048)
        n_mark, _, b_mark = ctx.profile_get("k_crop_mark")
        n_write, _, b_write = ctx.profile_get("k_crop_write")
        assert (n_mark, n_write, ctx.profile_get("k_crop_scan")[0]) == (1, 1, 1)
        assert b_mark == 12 * 16385 + mask and b_write == 12 * kept + mask
    finally:
        ctx.profile(False)
        ctx.profile_reset()


# ---- the service mirror ----------------------------------------------------------------------------
def _arm_poses():
    """Four camera -> arm frame transforms (origin, quaternion x y z w) that reach into a table scene
    seen from a camera about 1.3 m away."""
    rng = np.random.default_rng(23)
    poses = []
    for origin in ((-0.25, 0.05, 1.05), (0.2, 0.0, 1.1), (-0.3, -0.1, 1.3), (0.3, 0.1, 0.95)):
        q = Rotation.from_euler("xyz", rng.uniform(-1.0, 1.0, 3)).as_quat() * rng.uniform(0.5, 2.0)
        poses.append((origin, tuple(q)))
    return poses


def test_service_mirror(ctx):
    x, y, z = pitt.synth_frame(pitt.SCENE_TABLE_NAN, 1500, 160, 120)
    assert np.isnan(z).any()
    cloud = np.stack([x, y, z, np.ones_like(x)], 1)
    poses = _arm_poses()
    srv = pitt.Services(ctx)
    fmax, emin, emax = (0.30, 0.15, 0.11), (-0.10, -0.14, -0.15), (0.40, 0.14, 0.12)
    req = dict(forearm_min=(-1.0,), forearm_max=fmax, elbow_min=emin, elbow_max=emax)  # length 1: the default
    out, info = srv.arm_filter(cloud, poses, dense=False, **req)
    assert info["ok"]
    used = np.float32([FOREARM[0], fmax, emin, emax])
    assert np.array_equal(info["used"], used)
    boxes = info["boxes"]
    for k, (b, (origin, q)) in enumerate(zip(boxes, poses)):  # float64 geometry
        assert np.array_equal(np.float32(b.min[:]), used[0 if k < 2 else 2])
        assert np.array_equal(np.float32(b.max[:]), used[1 if k < 2 else 3])
        assert np.array_equal(np.float32(b.translation[:]), np.float32(origin))
        inv = Rotation.from_quat(q).as_matrix().T
        assert np.abs(np.array(b.inv_rotation[:], np.float64).reshape(3, 3) - inv).max() <= 1e-6
        assert b.has_rotation == 1 and b.has_translation == 1
    keep, removed = ref_crop(x, y, z, boxes, 1, False)
    assert (removed > 0).all() and removed[0] >= np.isnan(z).sum() and keep.sum() > 0
    assert np.array_equal(info["removed"], removed)
    assert np.array_equal(out.view(np.uint32), cloud[keep].view(np.uint32))
    # the device form
    dout, dinfo = srv.arm_filter_dev(*_dev(x, y, z), poses, dense=False, **req)
    assert np.array_equal(_bits(dout), cloud[keep][:, :3].view(np.uint32))
    assert np.array_equal(dinfo["removed"], removed) and np.array_equal(dinfo["used"], used)
    assert all(bytes(a) == bytes(b) for a, b in zip(dinfo["boxes"], boxes))
    # a transform error returns the input cloud
    cloud[:, 3] = np.random.default_rng(1).normal(size=len(x)).astype(np.float32)  # the pad travels too
    out, info = srv.arm_filter(cloud, poses, dense=False, tf_error=True, **req)
    assert out.tobytes() == cloud.tobytes() and not info["removed"].any() and info["ok"]
    assert np.array_equal(info["used"], used)
    dout, dinfo = srv.arm_filter_dev(*_dev(x, y, z), poses, dense=False, tf_error=True, **req)
    assert np.array_equal(_bits(dout), cloud[:, :3].view(np.uint32)) and not dinfo["removed"].any()
    srv.close()


# ---- the chain ---------------------------------------------------------------------------------------
def _pose(yaw_deg, pitch_deg, cam):
    """Camera optical frame -> z-up world frame, row-major 4x4 float (as tests/test_preprocess_gpu.py)."""
    yaw, pitch = np.radians(yaw_deg), np.radians(pitch_deg)
    f = np.array([np.sin(yaw) * np.cos(pitch), np.cos(yaw) * np.cos(pitch), -np.sin(pitch)])
    r = np.array([np.cos(yaw), -np.sin(yaw), 0.0])
    d = np.cross(f, r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, d, f, cam
    return m.astype(np.float32)


def test_chain_stays_on_the_device(ctx):
    """deepFiltering -> arm filter -> transformPointCloud -> findSupports (obj_segmentation.cpp:241-260)
    on device tensors, against the oracle chain with the restatement in the arm filter's place."""
    x, y, z = pitt.synth_frame(0, 1200, 320, 240)
    boxes = [pitt.crop_box(mn, mx, translation=o, rpy=Rotation.from_quat(q).as_euler("xyz"))
             for (mn, mx), (o, q) in zip((FOREARM, FOREARM, ELBOW, ELBOW), _arm_poses())]
    closer, _, used = ctx.deep_filter(*_dev(x, y, z), further=False)
    (ax, ay, az), removed = ctx.crop_boxes(*closer, boxes)
    m = _pose(0.0, 35.0, (0.0, 0.0, 1.35))
    wx, wy, wz = ctx.transform_cloud(ax, ay, az, m)
    dev = ctx.find_supports_dev(wx, wy, wz)

    rc, _ = orc.deep_filter(x, y, z, used)
    cx, cy, cz = (np.ascontiguousarray(a) for a in rc.T)
    keep, rrem = ref_crop(cx, cy, cz, boxes, 1, True)
    assert (rrem > 0).all() and np.array_equal(removed, rrem)
    rw = orc.transform_cloud(cx[keep], cy[keep], cz[keep], m)
    assert np.array_equal(_bits((wx, wy, wz)), rw.view(np.uint32))
    ref = orc.find_supports(*rw.T)
    assert len(dev) == len(ref) >= 1
    for d, r in zip(dev, ref):
        assert np.array_equal(d["idx_map"].cpu().numpy(), r["idx_map"])
        assert np.array_equal(d["coefficients"], r["coefficients"])
