"""Known answers of the lidar front end's restatement (tests/lidar_ref.py; specification: DESIGN.md section 1c) and of
input_pipeline.random_z_rotation.  CPU only."""
import math
import os

import numpy as np
import pytest
import torch

import lidar_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def vox(points, off, quant, rot=None):
    c, flagged = R.voxelise(np.asarray(points, dtype=np.float32), off, quant, rot)
    return c.tolist(), flagged


def test_floor_of_negatives_and_of_minus_zero():
    pts = [[-0.5, -0.0, 3.9], [-2.0, -2.0001, 1.9999], [-4.0, 4.0, -1e-30]]
    got, flagged = vox(pts, [0, 3], 2.0)
    assert got == [[0, -1, 0, 1], [0, -1, -2, 0], [0, -2, 2, -1]] and not flagged
    q, keep = R.quantise(np.array([[-0.0, -0.0, -0.0]], dtype=np.float32), 2.0)
    assert keep.all() and q.tolist() == [[0, 0, 0]]


def test_division_is_fp32_where_fp64_lands_in_another_voxel():
    # 4.5 / 0.3: fl32(0.3) = 0.300000012 and the fp32 quotient rounds to 14.999999 -> voxel 14; in fp64 4.5 / 0.3 = 15.000000000000002
    x = np.float32(4.5)
    assert np.floor(x / np.float32(0.3)) == 14.0 and np.floor(np.float64(x) / 0.3) == 15.0
    got, _ = vox([[4.5, 0.0, 0.0]], [0, 1], 0.3)
    assert got == [[0, 14, 0, 0]]
    # such points are not rare: the restatement follows fp32 on every one of them
    ks = [k for k in range(1, 400) if np.floor(np.float32(0.3 * k) / np.float32(0.3)) != np.floor(np.float64(np.float32(0.3 * k)) / 0.3)]
    assert len(ks) >= 10
    for k in ks:
        got, _ = vox([[np.float32(0.3 * k), 0.0, 0.0]], [0, 1], 0.3)
        assert got[0][1] == int(np.floor(np.float32(0.3 * k) / np.float32(0.3)))


def test_rotation_closed_form_at_0_and_90_degrees():
    pts = [[2.0, 4.0, 6.0], [-2.0, 8.0, -4.0]]                        # voxels (1, 2, 3), (-1, 4, -2) at quant_size 2
    eye = np.eye(3, dtype=np.float32)
    assert vox(pts, [0, 2], 2.0, eye)[0] == vox(pts, [0, 2], 2.0)[0] == [[0, 1, 2, 3], [0, -1, 4, -2]]
    r90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)      # (x, y, z) @ R = (y, -x, z)
    assert vox(pts, [0, 2], 2.0, r90)[0] == [[0, 2, -1, 3], [0, 4, 1, -2]]
    # the same angle through input_pipeline.z_rotation: cos(pi / 2) is 6.1e-17 in double precision, not 0, so a coordinate
    # that the exact matrix sends to 0 from a NEGATIVE x lands just below it -- floor(-6.1e-17) = -1.  The specification is the
    # arithmetic on the matrix it is given.
    from agplace_amd.input_pipeline import z_rotation
    rz = z_rotation(math.pi / 2).numpy()
    assert rz[0][1] == -1.0 and rz[1][0] == 1.0 and 0 < rz[0][0] < 1e-16
    assert vox([[2.0, 0.0, 0.0], [-2.0, 0.0, 0.0]], [0, 2], 2.0, rz)[0] == [[0, 0, -1, 0], [0, -1, 1, 0]]
    # per-sample matrices: sample 0 unrotated, sample 1 by 90 degrees
    both = np.stack([eye, r90])
    assert vox([pts[0], pts[0]], [0, 1, 2], 2.0, both)[0] == [[0, 1, 2, 3], [1, 2, -1, 3]]


def test_two_voxels_merge_under_a_5_degree_rotation():
    from agplace_amd.input_pipeline import z_rotation
    r5 = z_rotation(math.radians(5.0)).numpy()
    pts = [[0.5, 0.5, 0.5], [0.5, 2.5, 0.5]]                          # voxels (0, 0, 0) and (0, 1, 0)
    assert vox(pts, [0, 2], 2.0)[0] == [[0, 0, 0, 0], [0, 0, 1, 0]]
    got, _ = vox(pts, [0, 2], 2.0, r5)                                # (0, 1, 0) @ R = (sin 5, cos 5, 0) = (0.087, 0.996, 0) -> (0, 0, 0)
    assert got == [[0, 0, 0, 0], [0, 0, 0, 0]]
    assert R.merged(got).tolist() == [[0, 0, 0, 0]]


def test_equal_voxels_of_different_samples_stay_apart_and_duplicates_inside_one_merge():
    pts = [[1.0, 1.0, 1.0], [1.5, 0.5, 0.1], [1.0, 1.0, 1.0], [9.0, 1.0, 1.0]]
    got, _ = vox(pts, [0, 2, 4], 2.0)
    assert got == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 4, 0, 0]]


def test_drops_are_flagged_and_do_not_join_the_origin_voxel():
    pts = [[3.0, 3.0, 3.0], [float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0], [65024.0, 0.0, 0.0], [-65024.0, 0.0, 0.0],
           [65022.0, 0.0, 0.0], [-65023.0, 0.0, 0.0]]
    got, flagged = vox(pts, [0, 7], 2.0)
    assert flagged and got == [[0, 1, 1, 1], [0, 32511, 0, 0]]
    # |q| = 32512 is out (both signs), 32511 is the last one in; -65023 / 2 floors to -32512: out
    q, keep = R.quantise(np.array(pts, dtype=np.float32), 2.0)
    assert keep.tolist() == [True, False, False, False, False, True, False]
    # rows past off[B] are not looked at
    got, flagged = vox(pts, [0, 1], 2.0)
    assert got == [[0, 1, 1, 1]] and not flagged
    # a rotated voxel that leaves the range is dropped and flagged too
    r45 = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], dtype=np.float32)
    got, flagged = vox([[60000.0, 60000.0, 0.0], [2.0, 2.0, 0.0]], [0, 2], 2.0, r45)
    assert flagged and got == [[0, 2, 2, 0]]


def test_random_z_rotation_is_the_reference_matrix():
    from agplace_amd.input_pipeline import random_z_rotation, z_rotation
    g = torch.Generator().manual_seed(7)
    seen = []
    for _ in range(50):
        m = random_z_rotation(5.0, generator=g)
        assert m.dtype == torch.float32 and tuple(m.shape) == (3, 3)
        t = math.atan2(float(m[1, 0]), float(m[0, 0]))
        assert abs(t) <= math.radians(5.0) + 1e-7
        assert torch.equal(m, z_rotation(t)) or torch.allclose(m, z_rotation(t), atol=2 ** -24, rtol=0)
        assert m[2].tolist() == [0.0, 0.0, 1.0] and m[:, 2].tolist() == [0.0, 0.0, 1.0]
        assert float(m[0, 1]) == -float(m[1, 0]) and float(m[0, 0]) == float(m[1, 1])
        seen.append(t)
    assert min(seen) < -math.radians(2.0) and max(seen) > math.radians(2.0)          # both signs, most of the interval
    assert torch.equal(random_z_rotation(0.0), torch.eye(3))
    # the reference's own PCRandomRotation._M (scipy's matrix exponential of np.cross(np.eye(3), axis * theta), rounded to fp32) at
    # three fixed angles, recorded by tests/golden/make_pc_rotation.py.  Both sides round a double-precision value whose error
    # is a few 1e-16 to fp32, so they differ by at most one fp32 unit of the largest entries (2^-24 for values in [0.5, 1]).
    fx = np.load(os.path.join(GOLDEN, "pc_rotation.npz"))
    assert fx["matrix"].shape == (3, 3, 3)
    for theta, ref in zip(fx["theta"], fx["matrix"]):
        assert np.abs(z_rotation(float(theta)).numpy().astype(np.float64) - ref.astype(np.float64)).max() <= 2.0 ** -24
