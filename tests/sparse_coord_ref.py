"""The coordinate half of the sparse-voxel branch, restated without keys, sorting or binary searches: neighbour tables from a
Python dictionary (as oracle/sparse.py:conv builds them) and from a dense occupancy volume, the fp64 first convolution over such a
table, the window rule of conv0_mfma_kernel (csrc/sparse.hip) as a count per tile, and the named clouds of
tests/test_sparse_coord_ref.py (CPU: pins this file to the oracle) and tests/test_gpu_sparse_coord_kernels.py (the HIP entry
points agp_sparse_kernel_map_grid, agp_sparse_kernel_map and agp_sparse_conv0_fwd against it).

Coordinates are numpy int64 [n, 4] = (batch, x, y, z), rows sorted lexicographically and distinct; a table is int32
[len(offsets), n_out] whose entry [t][j] is the row of out[j] + offsets[t] among the input rows, `absent` when no such voxel
exists."""
import numpy as np
import torch

import sparse_kernel_ref as R

OFF, BITS = 1 << 15, 16                 # agplace_amd/sparse/coords.py: 16-bit fields, biased by 2^15
LIMIT = 32511                           # |coordinate| agp_sparse_build accepts without a range flag (headroom for kernel offsets)
PAD_KEY = 0x7fffffffffffffff            # what capacity-mode key arrays hold past their valid rows
C0_ROWS, C0_WK = 128, 1536              # csrc/sparse.hip: rows of a conv0_mfma_kernel tile, keys of a search window in LDS


# -------------------------------------------------------------------------------------------------------------------- keys
def keys_of(coords):
    """int64 [n, 4] (batch, x, y, z) -> int64 [n]: batch << 48 | x + 2^15 << 32 | y + 2^15 << 16 | z + 2^15"""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    assert c.size == 0 or (np.abs(c[:, 1:]).max() < OFF and c[:, 0].min() >= 0)
    return (c[:, 0] << (3 * BITS)) | ((c[:, 1] + OFF) << (2 * BITS)) | ((c[:, 2] + OFF) << BITS) | (c[:, 3] + OFF)


def coords_of(keys):
    """The inverse of keys_of."""
    k = np.asarray(keys, dtype=np.int64)
    f = (1 << BITS) - 1
    return np.stack([k >> (3 * BITS), ((k >> (2 * BITS)) & f) - OFF, ((k >> BITS) & f) - OFF, (k & f) - OFF], 1)


def key_offsets(offsets):
    """The key difference of every (dx, dy, dz): what agp_sparse_kernel_map takes as `dkey` (coords._dkeys)."""
    return np.array([(dx << (2 * BITS)) + (dy << BITS) + dz for dx, dy, dz in offsets], dtype=np.int64)


def seg_offsets(coords, nbatch):
    """int64 [nbatch + 1]: sample b owns rows [off[b], off[b + 1])"""
    cnt = np.bincount(np.asarray(coords)[:, 0], minlength=nbatch) if len(coords) else np.zeros(nbatch, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------- offsets
def offsets_centered(ksize, stride):
    """Odd kernel centred on the output: (i - ksize // 2) * stride per axis, kidx = ix + k * iy + k * k * iz."""
    assert ksize % 2 == 1
    r = ksize // 2
    return [((ix - r) * stride, (iy - r) * stride, (iz - r) * stride) for iz in range(ksize) for iy in range(ksize)
            for ix in range(ksize)]


def offsets_children(stride):
    """The 2 x 2 x 2 children of a stride-2 output on the level of `stride`: i * stride per axis, kidx = ix + 2 * iy + 4 * iz."""
    return [(ix * stride, iy * stride, iz * stride) for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)]


def offsets_up(stride):
    """What SparseTensor.up_map passes for the transposed convolution onto the level of `stride`: minus the child position."""
    return [(-ix * stride, -iy * stride, -iz * stride) for iz in (0, 1) for iy in (0, 1) for ix in (0, 1)]


def offsets_mixed(n=16, seed=0, reach=3):
    """`n` distinct offsets with components of both signs in [-reach, reach], in no particular order, (0, 0, 0) among them."""
    rng = np.random.default_rng(1000 + seed)
    seen = [(0, 0, 0), (reach, -reach, 1), (-reach, reach, -1)]
    while len(seen) < n:
        o = tuple(int(v) for v in rng.integers(-reach, reach + 1, 3))
        if o not in seen:
            seen.append(o)
    return [seen[i] for i in rng.permutation(n)]


# ------------------------------------------------------------------------------------------------------------------ tables
def table_dict(in_coords, out_coords, offsets, absent):
    """The table from a dictionary {(b, x, y, z): row}."""
    index = {tuple(c): i for i, c in enumerate(np.asarray(in_coords).tolist())}
    out = [tuple(c) for c in np.asarray(out_coords).tolist()]
    tab = np.empty((len(offsets), len(out)), dtype=np.int32)
    for t, (dx, dy, dz) in enumerate(offsets):
        tab[t] = [index.get((b, x + dx, y + dy, z + dz), absent) for b, x, y, z in out]
    return tab


def table_dense(in_coords, out_coords, offsets, absent):
    """The same table from a dense volume [B][X][Y][Z] of row numbers over the bounding box of the input voxels (translated to
    start at 0): vectorised, any cloud whose box fits in memory."""
    cin, cout = np.asarray(in_coords, dtype=np.int64).reshape(-1, 4), np.asarray(out_coords, dtype=np.int64).reshape(-1, 4)
    tab = np.full((len(offsets), cout.shape[0]), absent, dtype=np.int32)
    if cin.shape[0] == 0 or cout.shape[0] == 0:
        return tab
    lo, hi = cin.min(0), cin.max(0)
    ext = hi - lo + 1
    assert int(np.prod(ext)) <= 1 << 27, "bounding box %s: too large for a dense volume" % (ext,)
    vol = np.full(tuple(int(e) for e in ext), absent, dtype=np.int32)
    p = cin - lo
    vol[p[:, 0], p[:, 1], p[:, 2], p[:, 3]] = np.arange(cin.shape[0], dtype=np.int32)
    for t, (dx, dy, dz) in enumerate(offsets):
        q = cout + np.array([0, dx, dy, dz]) - lo
        ok = ((q >= 0) & (q < ext)).all(1)
        qq = q[ok]
        tab[t, ok] = vol[qq[:, 0], qq[:, 1], qq[:, 2], qq[:, 3]]
    return tab


def conv0_ref64(table, feats, w, scale=None, shift=None, relu=False):
    """The first voxel convolution (one input channel) in fp64: out[i] = relu?(scale * sum_t f[table[t][i]] w[t] + shift), absent
    entries = len(feats).  feats [n], w [ntaps, cout].  sparse_kernel_ref.conv_ref64 with cin = 1, on the device of `feats`."""
    f = feats.reshape(-1, 1)
    x = torch.cat([f, torch.zeros((1, 1), dtype=f.dtype, device=f.device)], 0)
    return R.conv_ref64(x, table, w.reshape(w.shape[0], 1, -1), scale, shift, None, relu)


# -------------------------------------------------------------------------------------------- the window of conv0_mfma_kernel
def tile_windows(keys, r, stride, rows=C0_ROWS):
    """int64 [ceil(n / rows)]: per tile of `rows` sorted rows, the number of keys from the first key >= keys[first] - span to the
    last key <= keys[last] + span, span = (r * stride) in all three coordinate fields -- the search window conv0_mfma_kernel copies
    into LDS when it holds at most C0_WK keys and searches in global memory otherwise."""
    k = np.asarray(keys, dtype=np.int64)
    rs = r * stride
    span = (rs << (2 * BITS)) + (rs << BITS) + rs
    first = np.arange(0, k.shape[0], rows)
    last = np.minimum(first + rows, k.shape[0]) - 1
    return np.searchsorted(k, k[last] + span, side="right") - np.searchsorted(k, k[first] - span, side="left")


# ------------------------------------------------------------------------------------------------------------------ clouds
def _sorted_unique(c):
    c = np.unique(np.asarray(c, dtype=np.int64).reshape(-1, 4), axis=0)          # (sorts lexicographically)
    return c


def window_end_keys_present(keys, r, stride, rows=C0_ROWS):
    """bool [tiles]: does the key keys[last] + span -- the last key a tile's window may hold -- exist?  Only then can a window
    whose upper bound is one key short be told from a right one."""
    k = np.asarray(keys, dtype=np.int64)
    rs = r * stride
    last = np.minimum(np.arange(0, k.shape[0], rows) + rows, k.shape[0]) - 1
    return np.isin(k[last] + ((rs << (2 * BITS)) + (rs << BITS) + rs), k)


def thin(seed=0):
    """-> (coords, nbatch = 3): samples 0 and 2 with about 440 distinct voxels each from [-14, 14)^3, sample 1 EMPTY.  The row
    count is no multiple of 128 and a tile of 128 rows straddles the two non-empty samples.  No tile's window ends ON a key
    (window_end_keys_present is False for every tile at reach 1, 2 and 3): the inclusive upper bound of the window is left to
    `slab`, whose interior tiles all end on one."""
    rng = np.random.default_rng(seed)
    while True:
        parts = []
        for b in (0, 2):
            p = rng.integers(-14, 14, size=(450, 3))
            parts.append(np.concatenate([np.full((450, 1), b), p], 1))
        c = _sorted_unique(np.concatenate(parts))
        n0 = int((c[:, 0] == 0).sum())
        k = keys_of(c)
        if c.shape[0] % 128 and n0 % 128 and not any(window_end_keys_present(k, r, 1).any() for r in (1, 2, 3)):
            return c, 3


def slab(seed=0):
    """-> (coords, nbatch = 4): sample 0 the FULL grid 6 x 24 x 24 (3456 voxels = 27 tiles of 128 rows; interior rows have every
    tap of a 5 x 5 x 5 kernel), samples 1 and 3 the two samples of thin(seed), sample 2 empty."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(24), np.arange(24), indexing="ij"), -1).reshape(-1, 3)
    t, _ = thin(seed)
    t = t.copy()
    t[:, 0] += 1
    return _sorted_unique(np.concatenate([np.concatenate([np.zeros((g.shape[0], 1), dtype=np.int64), g], 1), t])), 4


def edge(seed=0):
    """-> (coords, nbatch = 3): voxels at and next to +-LIMIT on every axis, every corner of the cube included, each with
    neighbours inside the reach of a 5 x 5 x 5 kernel; and the voxels a key-field borrow would reach if the fields had no
    headroom: for a voxel at z = -LIMIT the one at (y - 1, z = +LIMIT), for y = -LIMIT the one at (x - 1, y = +LIMIT), for
    x = -LIMIT the previous sample's x = +LIMIT -- neighbours in the SORTED order that are no neighbours in space."""
    rng = np.random.default_rng(seed + 77)
    pts = []
    for b in range(3):
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    corner = np.array([sx, sy, sz]) * LIMIT
                    pts.append((b, *corner))
                    for _ in range(5 if b != 1 else 2):                    # neighbours towards the inside, within 2 cells
                        d = rng.integers(0, 3, 3) * -np.array([sx, sy, sz])
                        pts.append((b, *(corner + d)))
        # along the faces: one axis at the limit, the others near the origin
        for axis in range(3):
            for s in (-1, 1):
                for _ in range(4):
                    p = rng.integers(-3, 4, 3)
                    p[axis] = s * (LIMIT - int(rng.integers(0, 3)))
                    pts.append((b, *p))
        # where a borrow would land
        pts += [(b, 5, 1, -LIMIT), (b, 5, 0, LIMIT), (b, 5, 0, LIMIT - 1), (b, 5, 1, -LIMIT + 1),
                (b, 1, -LIMIT, 2), (b, 0, LIMIT, 2), (b, 0, LIMIT, 1), (b, 1, -LIMIT + 1, 2),
                (b, -LIMIT, 0, 0), (b, LIMIT, 0, 0), (b, LIMIT, LIMIT, LIMIT - 1), (b, -LIMIT, -LIMIT, -LIMIT + 1)]
        pts += [(b, 0, 0, 0), (b, 0, 0, 1), (b, 1, 0, 0), (b, 0, -1, 0)]
    return _sorted_unique(np.array(pts, dtype=np.int64)), 3


def edge_translated(coords):
    """The edge cloud with every band of every axis moved next to the origin: c >= LIMIT - 40 -> c - (LIMIT - 100),
    c <= -(LIMIT - 40) -> c + (LIMIT - 100), |c| <= 10 unchanged.  The map is monotone per axis (the row order stays) and keeps
    every difference inside a band, while the bands stay 50 cells apart: the tables of offsets up to 50 cells are unchanged and
    table_dense's volume is 201 cells wide."""
    c = np.asarray(coords, dtype=np.int64).copy()
    s = c[:, 1:]
    a = np.abs(s)
    assert bool(((a <= 10) | (a >= LIMIT - 40)).all())
    c[:, 1:] = np.where(s >= LIMIT - 40, s - (LIMIT - 100), np.where(s <= -(LIMIT - 40), s + (LIMIT - 100), s))
    return c


def coarsen(coords, stride):
    """The coordinates of the level of `stride` (a power of two): every coordinate floored to a multiple, duplicates merged."""
    c = np.asarray(coords, dtype=np.int64).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], stride) * stride
    return _sorted_unique(c)


def levels(base, seed=0):
    """`base` in ("thin", "slab") -> ({1: coords, 2: coords, 4: coords}, nbatch): the cloud and its coarsened levels."""
    c, nb = {"thin": thin, "slab": slab}[base](seed)
    return {1: c, 2: coarsen(c, 2), 4: coarsen(c, 4)}, nb


def big(seed=0):
    """-> (coords, nbatch = 4): 35 000 distinct voxels in [0, 48)^3 per sample, 140 000 rows: more than the 131 072 rows (1024
    tiles) one round of conv0_mfma_kernel's grid covers, and with 16 offsets more than the 8192 x 256 threads of
    kernel_map_kernel's grid."""
    rng = np.random.default_rng(seed + 5)
    parts = []
    for b in range(4):
        cell = rng.choice(48 ** 3, size=35000, replace=False)
        parts.append(np.stack([np.full(cell.shape, b), cell // (48 * 48), cell // 48 % 48, cell % 48], 1))
    return _sorted_unique(np.concatenate(parts)), 4


CLOUDS = {"thin": thin, "slab": slab, "edge": edge, "big": big}
