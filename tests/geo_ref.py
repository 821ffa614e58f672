"""The oracle of the geo kernels (csrc/geo.hip): plain numpy fp64 restatements, the deliberately wrong variants that the
fixtures must tell apart from them, and the fixtures themselves (pure numpy, so that tests/test_geo_ref.py can evaluate the
wrong variants on the very inputs tests/test_gpu_geo.py gives the kernels)."""
import numpy as np

UTM0 = (368000.0, 140000.0)      # both exactly representable in float32 (spacing there: 1/32 m and 1/64 m)


# ------------------------------------------------------------------------------------------------ oracles
def radius_ref(q, db, radius, exclusive=False, arith=np.float64):
    """(offsets int64 [nq + 1], indices int64): per query the rows of db with dx*dx + dy*dy <= radius*radius, ascending.
    exclusive=True (`<`) and arith=np.float32 are the WRONG variants."""
    q = np.asarray(q).astype(arith).reshape(-1, 2)
    db = np.asarray(db).astype(arith).reshape(-1, 2)
    r2 = arith(radius) * arith(radius)
    counts = np.zeros(len(q), dtype=np.int64)
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(q), 256):
            dx = q[s:s + 256, None, 0] - db[None, :, 0]
            dy = q[s:s + 256, None, 1] - db[None, :, 1]
            d2 = dx * dx + dy * dy
            m = d2 < r2 if exclusive else d2 <= r2
            counts[s:s + 256] = m.sum(1)
            parts.append(np.nonzero(m)[1].astype(np.int64))          # row-major: ascending within every query
    off = np.zeros(len(q) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return off, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64))


def csr_lists(off, idx):
    return [idx[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def lists_csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    idx = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if off[-1] else np.zeros(0, dtype=np.int64)
    return off, idx


def first_hit_ref(pred, off, idx):
    """int32 [Q]: the first column j with pred[q][j] >= 0 and in list q, k if none."""
    k = pred.shape[1]
    out = np.full(len(pred), k, dtype=np.int32)
    for q, row in enumerate(pred):
        m = (row >= 0) & np.isin(row, idx[off[q]:off[q + 1]])
        if m.any():
            out[q] = np.argmax(m)
    return out


def first_hit_wrong_skips(pred, off, idx):
    """WRONG: takes the -1 entries out before counting columns."""
    k = pred.shape[1]
    out = np.full(len(pred), k, dtype=np.int32)
    for q, row in enumerate(pred):
        m = np.isin(row[row >= 0], idx[off[q]:off[q + 1]])
        if m.any():
            out[q] = np.argmax(m)
    return out


def first_hit_wrong_wraps(pred, off, idx, n_db):
    """WRONG: membership through a table indexed by the prediction, so that -1 reads the last database row."""
    k = pred.shape[1]
    out = np.full(len(pred), k, dtype=np.int32)
    for q, row in enumerate(pred):
        table = np.zeros(n_db, dtype=bool)
        table[idx[off[q]:off[q + 1]]] = True
        m = table[row]
        if m.any():
            out[q] = np.argmax(m)
    return out


def drop_listed_ref(I, cand, row_of_q, off, idx, negs, variant=None):
    """(out int64 [Q, negs], filled int32 [Q]): the first `negs` of cand[I[q]] not in list row_of_q[q], in I's order; the
    unfilled tail of `out` is -1 here (the kernel leaves it unwritten).
    WRONG variants: "position" tests the candidate POSITION against the list instead of its database row;
    "first_copy" removes only the first sampled copy of every listed row."""
    nq = len(I)
    out = np.full((nq, negs), -1, dtype=np.int64)
    filled = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        mine = idx[off[row_of_q[q]]:off[row_of_q[q] + 1]]
        p = I[q][(I[q] >= 0) & (I[q] < len(cand))]
        if variant == "position":
            keep = ~np.isin(p, mine)
        elif variant == "first_copy":
            _, first = np.unique(cand, return_index=True)
            dropped = first[np.isin(cand[first], mine)]
            keep = ~np.isin(p, dropped)
        else:
            keep = ~np.isin(cand[p], mine)
        rows = cand[p[keep]][:negs]
        out[q, :len(rows)] = rows
        filled[q] = len(rows)
    return out, filled


def knn_positions_ref(xq, xc, k):
    """[Q, k] positions of the k nearest rows of xc per query, exact fp64 squared distances, ties to the earlier position."""
    d = ((xq.astype(np.float64)[:, None, :] - xc.astype(np.float64)[None, :, :]) ** 2).sum(2)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int64)


# ------------------------------------------------------------------------------------------------ fixtures: radius
RADIUS_NB = (1, 63, 64, 65, 127, 1000, 4099)
RADIUS_NQ = (1, 3, 5, 257)


def _walk(rng, n, step=4.0):
    return np.cumsum(rng.normal(0.0, step, size=(n, 2)), 0) + np.asarray(UTM0)


def radius_cases():
    """[(name, q, db, radius)]: every nb x nq of the lists above on a random walk (float32 and float64 by turns; queries far
    away have empty lists), then the constructed cases."""
    cases = []
    for i, nb in enumerate(RADIUS_NB):
        for j, nq in enumerate(RADIUS_NQ):
            rng = np.random.default_rng(1000 + 10 * i + j)
            dt = np.float32 if (i + j) % 2 == 0 else np.float64
            db = _walk(rng, nb).astype(dt)
            q = (db[rng.integers(0, nb, nq)].astype(np.float64) + rng.normal(0.0, 6.0, size=(nq, 2)))
            q[::4] += 5000.0 * (np.arange(len(q[::4])) % 2)[:, None]            # every eighth query: nothing in reach
            cases.append((f"walk_nb{nb}_nq{nq}_{np.dtype(dt).name}", q.astype(dt), db, 25.0 if j % 2 else 10.0))
    rng = np.random.default_rng(7)
    db = _walk(rng, 1000).astype(np.float32)
    q = db[rng.integers(0, 1000, 5)] + np.float32(1.0)
    cases.append(("whole_database", q, db, 1.0e6))
    # lists of exactly 64 and 65: two tight clusters scattered over the rows of a 300-row database
    rng = np.random.default_rng(8)
    db = np.asarray(UTM0) + np.asarray([3000.0, 3000.0]) + rng.uniform(0, 1000, size=(300, 2))
    perm = rng.permutation(300)
    a, b = perm[:64], perm[64:129]
    db[a] = np.asarray(UTM0) + rng.uniform(-3, 3, size=(64, 2))
    db[b] = np.asarray(UTM0) + np.asarray([500.0, 0.0]) + rng.uniform(-3, 3, size=(65, 2))
    q = np.asarray([UTM0, (UTM0[0] + 500.0, UTM0[1]), (UTM0[0] + 250.0, UTM0[1])])
    cases.append(("lists_of_64_and_65", q, db, 10.0))
    # exact-boundary pairs: multiples of 3-4-5 at UTM offsets, float32 (the grid makes them exact), and their nearest outsiders
    pts = []
    for m in (1, 2, 3):
        pts += [(3 * m, 4 * m), (4 * m, 3 * m), (0, 5 * m), (5 * m, 0), (-3 * m, -4 * m), (0, -5 * m)]
    pts = np.asarray(pts, dtype=np.float64)
    out32 = np.asarray([(10 + 1 / 32, 0), (0, 10 + 1 / 64), (6 + 1 / 32, 8), (-10 - 1 / 32, 0)])
    db = (np.concatenate([pts, out32]) + np.asarray(UTM0)).astype(np.float32)
    q = np.asarray([UTM0], dtype=np.float32)
    cases.append(("boundary_f32_r10", q, db, 10.0))
    cases.append(("boundary_f32_r5", q, db, 5.0))
    cases.append(("boundary_f32_r15", q, db, 15.0))
    # the same in float64 with the next double beyond the boundary: float32 arithmetic folds it onto the boundary
    out64 = np.asarray([(np.nextafter(UTM0[0] + 10.0, np.inf), UTM0[1]), (UTM0[0], np.nextafter(UTM0[1] - 10.0, -np.inf)),
                        (np.nextafter(UTM0[0] + 6.0, np.inf), UTM0[1] + 8.0)])
    db = np.concatenate([pts + np.asarray(UTM0), out64])
    cases.append(("boundary_f64_r10", np.asarray([UTM0]), db, 10.0))
    cases.append(("three_four_five", np.asarray([(0.0, 0.0)]),
                  np.asarray([(3.0, 4.0), (0.0, 5.0), (5.0, 0.0), (np.nextafter(5.0, 6.0), 0.0)]), 5.0))
    # duplicate database points
    rng = np.random.default_rng(9)
    db = _walk(rng, 127).astype(np.float32)
    db[5] = db[70] = db[126] = db[0]
    db[64] = db[63]
    cases.append(("duplicates", db[[0, 63, 100]].copy(), db, 10.0))
    # one NaN and one inf row on each side
    rng = np.random.default_rng(10)
    db = _walk(rng, 65, step=2.0)
    q = db[[1, 2, 3, 4, 5]].copy()
    db[7] = (np.nan, UTM0[1])
    db[64] = (np.inf, np.inf)
    q[1] = (UTM0[0], np.nan)
    q[3] = (np.inf, UTM0[1])
    cases.append(("nan_inf_f64", q, db, 25.0))
    cases.append(("nan_inf_f32", q.astype(np.float32), db.astype(np.float32), 1.0e6))
    return cases


def sklearn_layout(seed=0):
    """The layout of the sklearn cross-check: a 2-D random walk of 20 000 float32 points at the UTM offset, 4096 queries
    perturbed from it."""
    rng = np.random.default_rng(seed)
    db = _walk(rng, 20000, step=3.0).astype(np.float32)
    q = (db[rng.integers(0, 20000, 4096)] + rng.normal(0.0, 8.0, size=(4096, 2)).astype(np.float32)).astype(np.float32)
    return q, db


# ------------------------------------------------------------------------------------------------ fixtures: first hit
FIRST_HIT_K = (1, 20, 64, 65, 1024)
FIRST_HIT_Q = (1, 63, 257)
N_DB = 20000
LIST_LENGTHS = (0, 1, 64, 65, 5000, 7)


def first_hit_case(k, nq, seed=0):
    """(pred int64 [nq, k], off, idx): lists of the lengths above by turns; predictions drawn from OUTSIDE the query's list, then
    hits planted at column 0, 63, 64, k - 1 or nowhere by turns (a second, later hit where there is room), -1 padding behind,
    and -1 entries IN FRONT of the planted hit for some queries, whose list then holds the last database row."""
    rng = np.random.default_rng(100 * k + nq + seed)
    lists, pred = [], np.empty((nq, k), dtype=np.int64)
    plant = (0, 63, 64, k - 1, None)
    for q in range(nq):
        n = LIST_LENGTHS[(q + nq) % len(LIST_LENGTHS)]
        pos = np.sort(rng.choice(N_DB - 1, size=n, replace=False)).astype(np.int64)
        front = q % 3 == 1 and n > 0
        if front:
            pos = np.append(pos, N_DB - 1)
        lists.append(pos)
        outside = np.setdiff1d(np.arange(N_DB, dtype=np.int64), pos, assume_unique=True)
        pred[q] = rng.choice(outside, size=k, replace=False)
        c = plant[(q // 2) % len(plant)]
        if c is not None and c < k and len(pos):
            pred[q, c] = pos[rng.integers(0, len(pos))]
            if c + 3 < k:
                pred[q, c + 3] = pos[0]
            if front and c >= 2:
                pred[q, :2] = -1
        if q % 4 == 2 and k > 4:
            pred[q, k - k // 4:] = -1                       # faiss's padding (may cover a planted k - 1: then no hit)
    off, idx = lists_csr(lists)
    return pred, off, idx


# ------------------------------------------------------------------------------------------------ fixtures: mining
class MiningFixture:
    """3000 database rows with d = 64 descriptors, 130 sampled queries out of 400, negs = 10.
    Rows [0, 80): cluster A within 3 m of query 0, descriptors next to query 0's -- all sampled in `cand` (1000 rows), so
    query 0's 64 nearest candidates are all soft positives; row 5 is sampled twice.
    Rows [80, 1180): cluster B within 20 m of query 1 -- 100 of them in `cand`, all 1100 in `cand_wide` (1200 rows), where
    query 1 exceeds MAX_K - negs.  Query 2 lies far from every row.  The rest is a random walk."""
    negs = 10

    def __init__(self):
        rng = np.random.default_rng(42)
        nd, nqall, d = 3000, 400, 64
        utm = _walk(rng, nd, step=15.0)
        qutm = utm[rng.integers(1180, nd, nqall)] + rng.normal(0.0, 5.0, size=(nqall, 2))
        feat = rng.standard_normal((nd, d)).astype(np.float32)
        qfeat = rng.standard_normal((nqall, d)).astype(np.float32)
        ca = np.asarray(UTM0) + np.asarray([-20000.0, 0.0])
        cb = np.asarray(UTM0) + np.asarray([0.0, -20000.0])
        utm[:80] = ca + rng.uniform(-2, 2, size=(80, 2))
        qutm[0] = ca
        feat[:80] = qfeat[0] + 0.01 * rng.standard_normal((80, d)).astype(np.float32)
        ang, rad = rng.uniform(0, 2 * np.pi, 1100), 20.0 * np.sqrt(rng.uniform(0, 1, 1100))
        utm[80:1180] = cb + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
        qutm[1] = cb
        feat[80:1180] = qfeat[1] + 0.5 * rng.standard_normal((1100, d)).astype(np.float32)
        qutm[2] = np.asarray(UTM0) + 1.0e5
        self.utm, self.qutm = utm.astype(np.float32), qutm.astype(np.float32)
        self.feat, self.qfeat_all = feat, qfeat
        self.sq = np.concatenate([[1, 0, 2], 3 + rng.choice(nqall - 3, size=127, replace=False)]).astype(np.int64)
        self.qfeat = qfeat[self.sq]
        rest = 1180 + rng.choice(nd - 1180, size=819, replace=False)
        cand = np.concatenate([np.arange(80), 80 + rng.choice(1100, size=100, replace=False), rest])
        cand = cand[rng.permutation(len(cand))]
        self.cand = np.insert(cand, 500, 5).astype(np.int64)                     # 1000 rows, row 5 twice
        wide = np.concatenate([np.arange(80, 1180), 1180 + rng.choice(nd - 1180, size=100, replace=False)])
        self.cand_wide = wide[rng.permutation(len(wide))].astype(np.int64)       # 1200 rows
        self.sq_wide = self.sq[:5]
        assert len(self.cand) == 1000 and len(self.sq) == 130

    def soft_ref(self):
        return radius_ref(self.qutm, self.utm, 25.0)

    def hard_ref(self):
        return radius_ref(self.qutm, self.utm, 10.0)
