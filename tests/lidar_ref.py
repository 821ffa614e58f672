"""numpy restatement of the lidar front end (TEST INFRASTRUCTURE; the specification is DESIGN.md section 1c): raw points ->
the (batch, x, y, z) voxel rows that level 0 of the sparse tensor is built from.  MinkowskiEngine is not available, so this
restates the reference's host chain (ME.utils.sparse_quantize per scan, batched_coordinates + PCRandomRotation in the collate
function) as the specification words it:

  quantise     q = floor(fl32(p / quant_size)) per axis -- a float32 array divided by a Python float is numpy's correctly rounded
               fp32 division; np.floor is a true floor (-0.25 -> -1, -0.0 -> 0)
  drop         rows with a non-finite component or |q| >= 32512 on an axis (flagged)
  deduplicate  one row per (b, qx, qy, qz), first occurrence kept; equal voxels of different samples stay apart
  rotate       c_j = floor((qx R[0][j] + qy R[1][j]) + qz R[2][j]) in fp64 from the integer q and the fp32 R, written out
               elementwise (no `@`: a BLAS product fixes no summation order); a rotated |c| >= 32512 drops the row (flagged)
Voxels that collide after the rotation are merged by the level-0 build itself (SparseTensor.from_coords on these rows)."""
import numpy as np

LIMIT = 32512


def quantise(points, quant_size):
    """points float32 [n, 3] -> (q int64 [n, 3], keep bool [n]); q is 0 where keep is False"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        qf = np.floor(p / float(quant_size))
        assert qf.dtype == np.float32
        keep = np.isfinite(p).all(1) & (np.abs(qf) < LIMIT).all(1)
    q = np.zeros(p.shape, dtype=np.int64)
    q[keep] = qf[keep].astype(np.int64)
    return q, keep


def rotate(q, rot):
    """q int64 [n, 3], rot float32 [3, 3] -> (c int64 [n, 3], keep bool [n]): floor of row vector x matrix in fp64"""
    r = np.asarray(rot)
    assert r.dtype == np.float32 and r.shape == (3, 3)
    r = r.astype(np.float64)
    qd = q.astype(np.float64)
    cf = np.empty(qd.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(3):
            cf[:, j] = np.floor((qd[:, 0] * r[0, j] + qd[:, 1] * r[1, j]) + qd[:, 2] * r[2, j])
        keep = (np.abs(cf) < LIMIT).all(1)          # (NaN compares False)
    c = np.zeros(q.shape, dtype=np.int64)
    c[keep] = cf[keep].astype(np.int64)
    return c, keep


def _sample_rot(rotation, b):
    if rotation is None:
        return None
    r = np.asarray(rotation)
    return r if r.ndim == 2 else r[b]


def voxelise(points, point_offsets, quant_size, rotation=None):
    """-> (coords int64 [m, 4] rows (b, cx, cy, cz): one per kept (b, q) in first-occurrence order, rotated; flagged bool).
    Only rows [off[b], off[b+1]) are read; rows from off[B] on are ignored."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    off = [int(v) for v in point_offsets]
    rows, flagged = [], False
    for b in range(len(off) - 1):
        q, keep = quantise(p[off[b]:off[b + 1]], quant_size)
        flagged = flagged or not bool(keep.all())
        q = q[keep]
        if len(q):
            _, first = np.unique(q, axis=0, return_index=True)
            q = q[np.sort(first)]
        r = _sample_rot(rotation, b)
        if r is not None and len(q):
            q, keep = rotate(q, r)
            flagged = flagged or not bool(keep.all())
            q = q[keep]
        rows.append(np.concatenate([np.full((len(q), 1), b, dtype=np.int64), q], 1))
    return (np.concatenate(rows, 0) if rows else np.zeros((0, 4), dtype=np.int64)), flagged


def per_point(points, point_offsets, quant_size, rotation=None):
    """The host chain WITHOUT the deduplication: int64 [n, 4] rows (b, cx, cy, cz), one per input row inside the offsets (every
    row must be in range) -- the `coords` a user of the parent library had to make on the host."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    off = [int(v) for v in point_offsets]
    rows = []
    for b in range(len(off) - 1):
        q, keep = quantise(p[off[b]:off[b + 1]], quant_size)
        assert keep.all()
        r = _sample_rot(rotation, b)
        if r is not None and len(q):
            q, keep = rotate(q, r)
            assert keep.all()
        rows.append(np.concatenate([np.full((len(q), 1), b, dtype=np.int64), q], 1))
    return np.concatenate(rows, 0)


def merged(coords):
    """sorted unique rows of `coords`: what the level-0 build keeps (lexicographic (b, x, y, z) order)"""
    return np.unique(np.asarray(coords, dtype=np.int64).reshape(-1, 4), axis=0)
