"""Host side of the device CropBox arm filter (no GPU): pitt_crop_box_from_rpy restates what PCL 1.7's
CropBox computes before its point loop (pcl::getTransformation in float, Eigen's 3x3 inverse, the fuzzy
isIdentity skip: DESIGN.md A12), and the service mirror's quaternion -> roll / pitch / yaw restates
tf::Matrix3x3::setRotation + getRPY in double (arm_filter_srv.cpp:77-79)."""
import ctypes

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import pitt_object_table_segmentation_amd as pitt
from pitt_object_table_segmentation_amd import _lib as L

FOREARM = ((-0.040, -0.120, -0.190), (0.340, 0.120, 0.105))  # arm_filter_srv.cpp:32-33


def _euler64(roll, pitch, yaw):
    """Rz(yaw) Ry(pitch) Rx(roll) in float64: the rotation pcl::getTransformation builds."""
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return rz @ ry @ rx


def test_record_layout():
    assert ctypes.sizeof(L.CropBox) == 80 and L.CropBox.has_translation.offset == 72
    b = pitt.crop_box(*FOREARM, translation=(0.1, 0.2, 0.3))
    assert np.array_equal(np.array(b.min[:]), np.float32(FOREARM[0]))
    assert np.array_equal(np.array(b.max[:]), np.float32(FOREARM[1]))
    assert np.array_equal(np.array(b.translation[:]), np.float32([0.1, 0.2, 0.3]))
    assert np.array_equal(np.array(b.inv_rotation[:]).reshape(3, 3), np.eye(3, dtype=np.float32))


def test_inverse_rotation_against_float64():
    """Each entry within 1e-6 of the float64 Euler rotation transposed: fewer than 16 float roundings of
    quantities <= 1 (cosf / sinf, the products and sums of an entry, the cofactor, the determinant and
    the scaling by its reciprocal), 16 * 2^-24 ~ 9.5e-7.  The float64 side starts from the same float
    angles the record was built from."""
    rng = np.random.default_rng(2024)
    worst = 0.0
    for rpy in rng.uniform(-np.pi, np.pi, (500, 3)):
        b = pitt.crop_box(*FOREARM, rpy=rpy)
        got = np.array(b.inv_rotation[:], np.float64).reshape(3, 3)
        ref = _euler64(*np.float32(rpy).astype(np.float64)).T
        worst = max(worst, np.abs(got - ref).max())
        assert b.has_rotation == 1
    print("worst |inv_rotation - float64|:", worst)
    assert worst <= 1e-6


def test_skip_flags():
    assert pitt.crop_box(*FOREARM, rpy=(0, 0, 0)).has_rotation == 0
    assert pitt.crop_box(*FOREARM, rpy=(-0.0, 0, -0.0)).has_rotation == 0
    # a non-zero rotation whose inverse is fuzzy-identity (Eigen isIdentity, precision 1e-5): PCL skips it
    assert pitt.crop_box(*FOREARM, rpy=(1e-6, 0, 0)).has_rotation == 0
    b = pitt.crop_box(*FOREARM, rpy=(1e-4, 0, 0))
    assert b.has_rotation == 1 and abs(b.inv_rotation[5] - 1e-4) < 1e-9
    for axis in range(3):  # off-diagonal 9e-6 passes the fuzzy test, 1.1e-5 does not
        small, big = [0.0] * 3, [0.0] * 3
        small[axis], big[axis] = 9e-6, 1.1e-5
        assert pitt.crop_box(*FOREARM, rpy=small).has_rotation == 0
        assert pitt.crop_box(*FOREARM, rpy=big).has_rotation == 1
    assert pitt.crop_box(*FOREARM, translation=(0, -0.0, 0)).has_translation == 0
    assert pitt.crop_box(*FOREARM, translation=(0, 1e-30, 0)).has_translation == 1
    assert pitt.crop_box(*FOREARM, translation=(0, 0, -2.5)).has_translation == 1
    assert pitt.crop_box(*FOREARM).has_translation == 0


def test_null_arguments_are_rejected_without_a_device():
    lib = L.lib
    v = (ctypes.c_float * 3)()
    b = L.CropBox()
    assert lib.pitt_crop_box_from_rpy(None, v, v, v, ctypes.byref(b)) == L.PITT_E_INVALID
    assert lib.pitt_crop_box_from_rpy(v, v, v, v, None) == L.PITT_E_INVALID
    n = ctypes.c_int64()
    assert lib.pitt_crop_boxes(None, None, None, None, 0, None, 0, 1, 1, None, None, None, ctypes.byref(n),
                               None) == L.PITT_E_INVALID
    assert lib.pitt_crop_boxes_host(None, None, 0, None, 0, 1, 1, None, ctypes.byref(n), None) == L.PITT_E_INVALID
    assert lib.pitt_srv_arm_filter(None, None, 0, 1, None, None, 0, None, ctypes.byref(n), None, None,
                                   None) == L.PITT_E_INVALID
    assert lib.pitt_srv_arm_filter_dev(None, None, None, None, 0, 1, None, None, 0, None, None, None, ctypes.byref(n),
                                       None, None, None) == L.PITT_E_INVALID
    assert lib.pitt_srv_quaternion_rpy(None, None) == L.PITT_E_INVALID


def test_quaternion_rpy_generic_poses():
    """tf's fixed-axis roll / pitch / yaw of R = Rz(yaw) Ry(pitch) Rx(roll) is scipy's 'xyz' (extrinsic)
    Euler triple; un-normalised quaternions too (setRotation scales by 2 / length2)."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in range(300):
        rpy = rng.uniform((-np.pi, -1.5, -np.pi), (np.pi, 1.5, np.pi))
        q = Rotation.from_euler("xyz", rpy).as_quat()  # x, y, z, w
        q = q * (1.0 if k % 3 else rng.uniform(0.3, 3.0)) * (1.0 if k % 2 else -1.0)
        got = pitt.quaternion_rpy(q)
        ref = Rotation.from_quat(q).as_euler("xyz")
        worst = max(worst, np.abs(got - ref).max())
    print("worst |rpy - scipy|:", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("q", [(0.5, 0.5, -0.5, 0.5), (0.5, -0.5, -0.5, -0.5), (0.0, 0.5, 0.0, 0.5),   # pitch = +pi/2
                               (0.5, -0.5, 0.5, 0.5), (-0.5, 0.5, -0.5, -0.5), (0.0, -2.0, 0.0, 2.0)])  # pitch = -pi/2
def test_quaternion_rpy_gimbal_lock(q):
    """At pitch = +-pi/2 only the rebuilt rotation is defined (tf sets yaw = 0).  The quaternions have
    components that make tf's m[2].x exactly -+1 in double, its gimbal branch; a pose a few ulps away
    takes the asin branch, whose conditioning there (d pitch ~ sqrt(2 ulp) ~ 2e-8) is tf's own."""
    roll, pitch, yaw = pitt.quaternion_rpy(q)
    assert abs(abs(pitch) - np.pi / 2) <= 1e-15 and yaw == 0.0
    want = Rotation.from_quat(q).as_matrix()
    assert np.abs(_euler64(roll, pitch, yaw) - want).max() <= 1e-12
