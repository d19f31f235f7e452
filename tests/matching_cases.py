"""The case catalogue and the references of the evaluation path's tests (NumPy only): the nearest-neighbour search, the
mutual check with its inlier count, the keypoint selection and RANSAC, each at the edges of its kernels
(csrc/matching.hip, keypoints.hip, ransac.hip).  tests/test_matching_cases_host.py proves the catalogue on the CPU (every
case meets its conditions, the references agree with imf_oracle on generic data); tests/test_gpu_matching_exact.py runs
the kernels against it.

The nearest-neighbour reference is exact arithmetic on the float32 inputs (Python integers after scaling every value by
one power of two).  The gates are stated on the bound

    E(q, d) = 2 (dim + 2) 2^-53 (|q| + |d|)^2.

Derivation.  The device forms s = |d|^2 - 2 q.d in fp64.  A product of two float32 values has 48 significant bits and is
exact in fp64, so only additions round: dim - 1 for the norm |d|^2, then a (dim + 1)-term accumulation of the norm and
the dim products.  No term passes through more than 2 dim - 1 additions, each of relative error u = 2^-53, so
|s - exact| <= g (|d|^2 + 2 sum |q_c d_c|) with g = (2 dim - 1) u / (1 - (2 dim - 1) u) (the standard bound of recursive
summation, which holds for every order of the additions).  Cauchy-Schwarz gives sum |q_c d_c| <= |q| |d|, so
|d|^2 + 2 |q| |d| <= (|q| + |d|)^2, and g <= 2 (dim + 2) u: |s - exact| <= E(q, d).  It is a bound, not a measurement."""
import functools
from fractions import Fraction
from typing import NamedTuple, Optional

import numpy as np

import imf_oracle as O

U53 = 2.0 ** -53
I32_MAX = 2 ** 31 - 1


# ---- nearest neighbour -------------------------------------------------------------------------------------------------
def nn_splits(nq, nd):
    """(splits, split_len) of imf_nn_search, restated from csrc/matching.hip: enough workgroups for 512, at most one
    split per 64-row tile, at most 64; the split length a multiple of the tile."""
    blocks = -(-nq // 64) if nq > 0 else 1
    s = max(1, min(-(-512 // blocks), -(-nd // 64), 64))
    return s, -(-(-(-nd // s)) // 64) * 64


def bound_E(q, d):
    """E(q, d) of the module docstring for one query row against rows d [n, dim] (or one row), in fp64."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    return 2.0 * (q.shape[-1] + 2) * U53 * (np.sqrt((q * q).sum(-1)) + np.sqrt((d * d).sum(-1))) ** 2


def exact_ints(*arrays):
    """float32 arrays -> (object arrays of Python integers, e) with every x == int * 2^e exactly."""
    xs = [np.asarray(a, np.float32).astype(np.float64) for a in arrays]
    parts = [np.frexp(x) for x in xs]                                         # x = m 2^ex, m 2^24 an integer for a float32
    exps = [ex[x != 0] - 24 for x, (_, ex) in zip(xs, parts)]
    exps = np.concatenate([e.ravel() for e in exps])
    e = int(exps.min()) if exps.size else 0
    out = []
    for x, (m, ex) in zip(xs, parts):
        mi = (m * 2.0 ** 24).astype(np.int64).ravel()
        sh = np.where(x.ravel() != 0, ex.ravel() - 24 - e, 0)
        out.append(np.array([int(a) << int(s) for a, s in zip(mi, sh)], dtype=object).reshape(x.shape))
    return out, e


class NNRef(NamedTuple):
    argmin: np.ndarray          # int64 [nq]: the exact nearest row, the lowest index on exact ties
    pinned: np.ndarray          # bool [nq]: the exact gap to the second distinct distance exceeds E(best) + E(second)
    qi: np.ndarray              # the exact integers of q and d, and their common exponent
    di: np.ndarray
    e: int
    first_equal: np.ndarray     # int64 [nd]: the lowest index of a row bitwise equal to row j


def _d2_int(qi_row, di_rows):
    return ((di_rows - qi_row) ** 2).sum(-1)


def nn_reference(q, d):
    """The exact 1-NN of every float32 row of q among the float32 rows of d (all finite).  An fp64 sum((q - d)^2)
    pre-pass picks the candidates: the 4 nearest and every row within 4 E of the fp64 minimum (the pre-pass is itself
    within E of the exact value, so the exact argmin and, unless the query is pinned anyway, the exact second distinct
    distance are among them); exact integer arithmetic decides between them."""
    q, d = np.asarray(q, np.float32), np.asarray(d, np.float32)
    assert np.isfinite(q).all() and np.isfinite(d).all()
    (qi, di), e = exact_ints(q, d)
    q64, d64 = q.astype(np.float64), d.astype(np.float64)
    nq, nd = len(q), len(d)
    dn_max = np.sqrt((d64 * d64).sum(1)).max()
    argmin, pinned = np.empty(nq, np.int64), np.empty(nq, bool)
    scale = Fraction(2) ** (2 * e)
    for i in range(nq):
        d2 = ((d64 - q64[i]) ** 2).sum(1)
        e_max = 2.0 * (q.shape[1] + 2) * U53 * (np.sqrt((q64[i] ** 2).sum()) + dn_max) ** 2
        k = min(nd, 4)
        cand = np.union1d(np.argpartition(d2, k - 1)[:k], np.flatnonzero(d2 <= d2.min() + 4.0 * e_max))
        D = _d2_int(qi[i], di[cand])
        best = min(D)
        a = int(cand[[x == best for x in D].index(True)])
        argmin[i] = a
        further = [x for x in D if x > best]
        if not further:
            pinned[i] = True                                                   # every other row is beyond the window
            continue
        second = min(further)
        e2 = max(float(bound_E(q64[i], d64[int(c)])) for c, x in zip(cand, D) if x == second)
        pinned[i] = (second - best) * scale > Fraction(float(bound_E(q64[i], d64[a]))) + Fraction(e2)
    seen, first_equal = {}, np.empty(nd, np.int64)
    for j in range(nd):
        first_equal[j] = seen.setdefault(d[j].tobytes(), j)
    return NNRef(argmin, pinned, qi, di, e, first_equal)


def nn_gate(q, d, ref, got_idx, got_d2=None):
    """The gates of the issue for one search; returns a list of failure strings (empty = pass).
    Index: in range; the lowest index among bitwise equal rows; d2_exact(q, got) <= d2_exact(q, argmin) + E(q, got) +
    E(q, argmin) everywhere; equal to the exact argmin where the query is pinned.  dist2: within 2 E(q, got) of the exact
    squared distance of the row returned."""
    q64, d64 = np.asarray(q, np.float64), np.asarray(d, np.float64)
    scale = Fraction(2) ** (2 * ref.e)
    bad = []
    for i in range(len(q64)):
        g, a = int(got_idx[i]), int(ref.argmin[i])
        if not 0 <= g < len(d64):
            bad.append(f"query {i}: index {g} out of range")
            continue
        if ref.first_equal[g] != g:
            bad.append(f"query {i}: row {g} has a bitwise equal row {ref.first_equal[g]} below it")
        Eg, Ea = Fraction(float(bound_E(q64[i], d64[g]))), Fraction(float(bound_E(q64[i], d64[a])))
        Dg = _d2_int(ref.qi[i], ref.di[g]) * scale
        Da = _d2_int(ref.qi[i], ref.di[a]) * scale
        if Dg > Da + Eg + Ea:
            bad.append(f"query {i}: row {g} is {float(Dg - Da):.3e} further than the nearest row {a}, E sum {float(Eg + Ea):.3e}")
        if ref.pinned[i] and g != a:
            bad.append(f"query {i}: pinned to row {a}, got {g}")
        if got_d2 is not None:
            v = float(got_d2[i])
            if not np.isfinite(v) or abs(Fraction(v) - Dg) > 2 * Eg:
                bad.append(f"query {i}: dist2 {v!r} against exact {float(Dg)!r}, 2E {float(2 * Eg):.3e}")
    return bad


class NNCase(NamedTuple):
    name: str
    q: np.ndarray               # float32 [nq, dim]
    d: np.ndarray               # float32 [nd, dim]
    kind: str                   # "generic" (capped pinned share), "tie", "zero", "mixed", "nonfinite"
    splits: int                 # what nn_splits gives for this shape, written out
    split_len: int
    want: Optional[np.ndarray] = None       # tie / zero cases: the index every query must return


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


NQ_EDGES = (1, 15, 16, 17, 63, 64, 65)                     # wave of 16 query columns, workgroup of 64
ND_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)      # 16-row block, 64-row tile
# nd -> (splits, split_len) for nq <= 65 (one or two workgroups: the tile count is what limits the splits)
EDGE_SPLITS = {1: (1, 64), 15: (1, 64), 16: (1, 64), 17: (1, 64), 63: (1, 64), 64: (1, 64), 65: (2, 64), 127: (2, 64),
               128: (2, 64), 129: (3, 64)}
# (nq, nd) -> (splits, split_len): 64 splits of 128 of which 31 are empty; two splits, the second of 6 rows
BIG_SPLITS = {(129, 4097): (64, 128), (1000, 70): (2, 64)}


def nn_shape_cases():
    out = []
    for dim in (16, 32, 64):
        for nq in NQ_EDGES:
            for nd in ND_EDGES:
                rng = np.random.default_rng(dim * 100003 + nq * 1009 + nd)
                out.append(NNCase(f"shape_d{dim}_q{nq}_n{nd}", unit_rows(rng, nq, dim), unit_rows(rng, nd, dim), "generic",
                                  *EDGE_SPLITS[nd]))
    for (nq, nd), sp in BIG_SPLITS.items():
        for dim in ((16, 32, 64) if nq == 129 else (32,)):
            rng = np.random.default_rng(dim * 100003 + nq * 1009 + nd)
            out.append(NNCase(f"shape_d{dim}_q{nq}_n{nd}", unit_rows(rng, nq, dim), unit_rows(rng, nd, dim), "generic", *sp))
    return out


# Tie layouts: (nq, nd) with their (splits, split_len).  200 rows are 4 splits of one tile each; 4097 rows against 129
# queries are splits of two tiles, so "next tile" stays inside a split there.
TIE_LAYOUTS = {(20, 200): (4, 64), (129, 4097): (64, 128)}


def tie_pairs(nd, split_len):
    i = 5
    return {"next_lane": (i, i + 1), "next_register": (i, i + 4), "next_block": (i, i + 16), "next_tile": (i, i + 64),
            "across_split": (split_len - 1, split_len), "first_last": (0, nd - 1)}


def nn_tie_cases():
    """Two bitwise equal rows, both nearest to every query, at chosen positions.  Arrangement "far": every other row is
    a random unit vector, about 1 away, so a lane's first candidate is rarely its last; "near": every other row sits in
    a shell just outside the pair, so every lane, block and split offers a close competitor.  The expected answer is the
    lower index of the pair for every query."""
    out = []
    for (nq, nd), (splits, split_len) in TIE_LAYOUTS.items():
        for pname, (a, b) in tie_pairs(nd, split_len).items():
            for arr in ("far", "near"):
                rng = np.random.default_rng(nd * 31 + a * 7 + b + (arr == "near"))
                v = unit_rows(rng, 1, 32)[0]
                if arr == "far":
                    d = unit_rows(rng, nd, 32)
                    d[a] = d[b] = v
                    q = v + (0.05 * unit_rows(rng, nq, 32))
                else:
                    d = v + unit_rows(rng, nd, 32) * rng.uniform(0.10, 0.15, (nd, 1)).astype(np.float32)
                    d[a] = d[b] = v + 0.05 * unit_rows(rng, 1, 32)[0]
                    q = v + (0.01 * unit_rows(rng, nq, 32))
                out.append(NNCase(f"tie_{pname}_{arr}_n{nd}", q.astype(np.float32), d.astype(np.float32), "tie", splits,
                                  split_len, np.full(nq, a, np.int64)))
    return out


def nn_zero_cases():
    """A zero query (and two tiny ones) against rows of distinct positive norms.  The rows the kernel stages past the end
    of a split are zero and score 0 < |d|^2: they must not win.  nd = 65 and 4097 are split_len + 1 (the last split holds
    one row and 63 or 127 staged zero rows); nd = 1 is one row and 63 zero rows."""
    out = []
    for nq, nd in ((3, 1), (3, 65), (129, 4097)):
        rng = np.random.default_rng(nd)
        d = unit_rows(rng, nd, 32) * np.float32(2.0) ** rng.integers(0, 3, (nd, 1)).astype(np.float32)
        d *= (1.0 + np.arange(nd, dtype=np.float32)[:, None] / np.float32(8192.0))
        lo = int(rng.integers(0, nd))
        d[lo] *= np.float32(0.25)                                                # the row of the smallest norm
        q = np.zeros((nq, 32), np.float32)
        q[1:] = (1e-3 * unit_rows(rng, nq - 1, 32))
        splits, split_len = nn_splits(nq, nd)
        out.append(NNCase(f"zero_q{nq}_n{nd}", q, d.astype(np.float32), "zero", splits, split_len, np.full(nq, lo, np.int64)))
    return out


# Pinned shares of the mixed-magnitude cases, measured with nn_reference (test_matching_cases_host.py prints them; no cap
# is set for them): shared_component 1.000, scaled_2^-60 1.000, scaled_2^40 1.000.
def nn_mixed_cases():
    out = []
    rng = np.random.default_rng(77)

    def shared(n):
        x = rng.uniform(0.5, 1.5, (n, 32))
        x[:, 0] = 1000.0 + rng.uniform(-0.5, 0.5, n)                             # one component near 10^3, full mantissas
        return x.astype(np.float32)
    out.append(NNCase("mixed_shared_component", shared(70), shared(300), "mixed", *nn_splits(70, 300)))
    for name, s in (("mixed_scaled_2^-60", 2.0 ** -60), ("mixed_scaled_2^40", 2.0 ** 40)):
        q, d = unit_rows(rng, 70, 32), unit_rows(rng, 300, 32)
        out.append(NNCase(name, (q * np.float32(s)).astype(np.float32), (d * np.float32(s)).astype(np.float32), "mixed",
                          *nn_splits(70, 300)))
    return out


class NonFiniteCase(NamedTuple):
    name: str
    q: np.ndarray
    d: np.ndarray
    bad_q: np.ndarray           # bool [nq]: queries that must answer (-1, NaN)
    bad_d: np.ndarray           # bool [nd]: rows that must never be chosen


def nn_nonfinite_cases():
    """One generic search (40 x 150 x 32, three splits) with non-finite values planted: in query rows (at a wave edge and
    the last row, in the first and the last component), in database rows (first, around a tile and split edge, last),
    and a database without one finite row.  Components of the finite rows have both signs, so an infinite entry meets
    products of both signs."""
    rng = np.random.default_rng(4242)
    q0, d0 = unit_rows(rng, 40, 32), unit_rows(rng, 150, 32)
    out = []
    for vname, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        q = q0.copy()
        q[0, 0] = q[15, 31] = q[16, 7] = q[39, 31] = v
        out.append(NonFiniteCase(f"query_{vname}", q, d0, ~np.isfinite(q).all(1), np.zeros(150, bool)))
        d = d0.copy()
        d[0, 31] = d[63, 0] = d[64, 5] = d[149, 31] = v
        out.append(NonFiniteCase(f"db_{vname}", q0, d, np.zeros(40, bool), ~np.isfinite(d).all(1)))
    d = d0.copy()
    d[:, 3] = np.nan
    d[1::3, 3] = np.inf
    d[2::3, 3] = -np.inf
    out.append(NonFiniteCase("db_all_nonfinite", q0, d, np.ones(40, bool), np.ones(150, bool)))
    q = q0.copy()
    q[3, 2] = np.inf
    q[4, 2] = np.nan
    d = d0.copy()
    d[10, 2] = -np.inf
    d[11, 2] = np.nan
    d[12, 2] = 0.0                                                                # inf * 0 in the product
    out.append(NonFiniteCase("both_sides", q, d, ~np.isfinite(q).all(1), ~np.isfinite(d).all(1)))
    return out


# ---- mutual check and inliers ------------------------------------------------------------------------------------------
class MutualCase(NamedTuple):
    name: str
    nn21: np.ndarray            # int32 [n2]
    nn12: np.ndarray            # int32 [n1]
    kp1: Optional[np.ndarray]   # float64 [n1, 3] or None
    kp2: Optional[np.ndarray]
    pose: Optional[np.ndarray]
    thresh: float


def mutual_reference(c):
    """scripts/evaluation_3dmatch.py:212-234 as imf_oracle states it, with the rule that an nn21 entry outside [0, n1) is
    never a match: (match2 int32 ascending, n_inliers)."""
    nn21, nn12 = np.asarray(c.nn21, np.int64), np.asarray(c.nn12, np.int64)
    n2, n1 = len(nn21), len(nn12)
    ok = (nn21 >= 0) & (nn21 < n1)
    m2 = np.flatnonzero(ok & (nn12[np.where(ok, nn21, 0)] == np.arange(n2))) if n1 else np.zeros(0, np.int64)
    if c.kp1 is None:
        return m2.astype(np.int32), 0
    k2 = O.transform_points(c.kp2[m2], c.pose)
    dist = np.sqrt(np.sum(np.square(c.kp1[nn21[m2]] - k2), axis=1))
    return m2.astype(np.int32), int(np.sum(dist < c.thresh))


MUTUAL_N2 = (1, 63, 64, 65, 1023, 1024, 1025, 2049)        # chunk of 1 024, wave of 64
QUARTER_POSE = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.125], [0.0, 0.0, 0.0, 1.0]])
INVALID_NN = (-1, None, I32_MAX)                           # None stands for n1


def _lattice_points(rng, n):
    return rng.integers(-64, 64, (n, 3)).astype(np.float64) / 8.0              # dyadic: every distance^2 is exact in fp64


def mutual_cases():
    """Keypoints on a dyadic lattice under a quarter turn with a dyadic translation: the transformed points, the
    differences and the squared distances are exact in fp64 whatever the order or fusing of the operations, so the
    inlier count is exact on both sides.  kp1[nn21[j]] = pose . kp2[j] + (0 or one lattice step), thresh 0.1."""
    out = []
    for n2 in MUTUAL_N2:
        for pat in ("all", "none", "chunk_edges"):
            rng = np.random.default_rng(n2 * 3 + len(pat))
            n1 = n2 + 2
            perm = rng.permutation(n1)[:n2].astype(np.int64)                  # nn21: injective into [0, n1)
            nn21 = perm.copy()
            nn12 = np.full(n1, -1, np.int64)
            if pat == "all":
                nn12[perm] = np.arange(n2)
            elif pat == "none":
                nn12[perm] = (np.arange(n2) + 1) % n2 if n2 > 1 else -1
                nn12[nn12 == -1] = n2                                          # an index that is nobody's
            else:
                keep = sorted({j for c0 in range(0, n2, 1024) for j in (c0, min(c0 + 1023, n2 - 1))})
                nn12[perm] = (np.arange(n2) + 1) % max(n2, 2)
                nn12[perm[keep]] = keep
            if pat != "none" and n2 >= 63:                                     # entries that are no index of frag1
                for k, v in zip((1, 30, n2 // 2 + 1, n2 - 3), INVALID_NN + (-1,)):
                    nn21[k] = n1 if v is None else v
            kp2 = _lattice_points(rng, n2)
            kp1 = _lattice_points(rng, n1)
            ok = (nn21 >= 0) & (nn21 < n1)
            moved = O.transform_points(kp2, QUARTER_POSE)
            step = np.where(rng.random((n2, 1)) < 0.5, 0.0, 0.125) * np.eye(3)[rng.integers(0, 3, n2)]
            kp1[nn21[ok]] = (moved + step)[ok]
            out.append(MutualCase(f"n{n2}_{pat}", nn21.astype(np.int32), nn12.astype(np.int32), kp1, kp2, QUARTER_POSE, 0.1))
    one = np.zeros(1, np.int32)
    k1, k2 = np.zeros((1, 3)), np.array([[0.375, 0.5, 0.0]])                    # |kp2| = 0.625 exactly
    out.append(MutualCase("strict_at_equality", one, one, k1, k2, np.eye(4), 0.625))
    out.append(MutualCase("strict_above_equality", one, one, k1, k2, np.eye(4), float(np.nextafter(0.625, 1.0))))
    for w in (2.0, 0.5):                                                       # projective: divide by w
        T = QUARTER_POSE.copy()
        T[3, 3] = w
        rng = np.random.default_rng(int(w * 10))
        kp2 = _lattice_points(rng, 65)
        kp1 = O.transform_points(kp2, T)
        kp1[::2] += [0.0, 0.125, 0.0]
        out.append(MutualCase(f"projective_w{w}", np.arange(65, dtype=np.int32), np.arange(65, dtype=np.int32), kp1, kp2, T, 0.1))
    out.append(MutualCase("no_geometry_n2049", *out[MUTUAL_N2.index(2049) * 3 + 2][1:3], None, None, None, 0.1))
    return out


# ---- keypoint selection ------------------------------------------------------------------------------------------------
class KeypointCase(NamedTuple):
    name: str
    samples: np.ndarray         # float64 [ns, 3]
    coords: np.ndarray          # float64 [m, 3]
    voxel: float


def hash64(k):
    """common.h hash64 on a Python integer key: the first slot of a key in a key-only set is hash64(k) & (capacity - 1)."""
    M = (1 << 64) - 1
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M
    k ^= k >> 33
    return k & 0xFFFFFFFF


def hash_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def cell_key(cell):
    """The FNV key of one integer cell, as a Python integer."""
    return int(O.fnv_hash_vec(np.asarray([cell], np.float64))[0])


@functools.lru_cache(maxsize=None)
def colliding_cells():
    """Two distinct cells (0, 0, a) and (0, 0, b) whose keys differ and share the first slot of a 1024-slot set."""
    seen = {}
    for z in range(100000):
        k = cell_key((0, 0, z))
        s = hash64(k if k != (1 << 64) - 1 else (1 << 64) - 2) & 1023
        if s in seen and seen[s][1] != k:
            return (0, 0, seen[s][0]), (0, 0, z)
        seen.setdefault(s, (z, k))
    raise AssertionError("no colliding pair found")


KP_M = (0, 1, 1023, 1024, 1025, 2049)                      # block of 1 024 rows in probe / scan / emit


def keypoint_cases():
    out = []
    v = 0.05
    for m in KP_M:
        rng = np.random.default_rng(500 + m)
        coords = rng.uniform(-3.0, 3.0, (m, 3))
        out.append(KeypointCase(f"m{m}_ns0", np.zeros((0, 3)), coords, v))
        one = coords[m // 2][None] if m else np.array([[0.1, 0.2, 0.3]])
        out.append(KeypointCase(f"m{m}_ns1", one.copy(), coords, v))
        out.append(KeypointCase(f"m{m}_all_selected", coords.copy(), coords, v))
        out.append(KeypointCase(f"m{m}_none_selected", coords + 1000.0, coords, v))
        if m > 1:                                                               # the first and last row of every block only
            rows = sorted({r for b in range(0, m, 1024) for r in (b, min(b + 1023, m - 1))})
            c2 = coords.copy()
            c2[rows] += 500.0
            out.append(KeypointCase(f"m{m}_block_edges", c2[rows].copy(), c2, v))
    rng = np.random.default_rng(9)
    coords = rng.uniform(-1.0, 1.0, (1500, 3))
    out.append(KeypointCase("repeated_samples", np.tile(coords[[3, 700, 1499]], (100, 1)), coords, v))
    neg = np.array([[-0.0, 0.0, -0.0], [-0.05, -0.0, 0.05], [-1e-9, -0.05 - 1e-9, 0.1], [0.049999, -0.1, 0.0],
                    [-0.025, -0.025, -0.025], [-2.5, -3.0, -0.0]])
    out.append(KeypointCase("negative_and_minus_zero", np.array([[0.0, -0.0, 0.0], [-0.01, -0.01, -0.01], [-2.51, -3.0, 0.01]]),
                            neg, v))
    # 0.15 / 0.05 = 2.9999999999999996 in fp64: the point on the face of cell 3 belongs to cell 2 (and -0.15 to cell -3)
    face = np.array([[0.15, 0.15, 0.15], [-0.15, -0.15, -0.15], [0.1499, 0.1499, 0.1499], [0.151, 0.151, 0.151],
                     [-0.151, -0.151, -0.151], [0.15, -0.15, 0.151]])
    out.append(KeypointCase("face_quotient_rounds_below", np.array([[0.12, 0.12, 0.12], [-0.14, -0.14, -0.14], [0.16, -0.16, 0.16]]),
                            face, v))
    big = np.array([[2.0 ** 31, 0.0, 0.0], [2.0 ** 31 + 1, 0.0, 0.0], [-(2.0 ** 31) - 1, 0.0, 0.0], [2.0 ** 33 + 0.5, -(2.0 ** 40), 1.0],
                    [2.0 ** 52 - 1, 0.0, 0.0], [2.0 ** 52 - 2, 0.0, 0.0], [-(2.0 ** 52) + 1, 0.0, 0.0], [-(2.0 ** 52) + 2, 5.0, 0.0],
                    [0.0, 2.0 ** 52 - 1, -(2.0 ** 52) + 1], [3.0, 3.0, 3.0]])
    out.append(KeypointCase("quotients_beyond_2^31_and_near_2^52", big[[1, 2, 4, 7, 8]].copy() + [0.25, 0.0, 0.0], big, 1.0))
    out.append(KeypointCase("quotients_scaled_voxel", big[[0, 3, 6]].copy() * 0.5, big * 0.5, 0.5))
    a, b = colliding_cells()
    ca, cb = (np.array(a) + 0.5) * v, (np.array(b) + 0.5) * v
    other = np.array([[0.31, 0.32, 7.7]])
    out.append(KeypointCase("shared_slot_absent_key", ca[None].copy(), np.stack([cb, ca, cb, other[0]]), v))
    out.append(KeypointCase("shared_slot_both_present", np.stack([ca, cb]), np.stack([cb, other[0], ca]), v))
    out.append(KeypointCase("shared_slot_other_order", cb[None].copy(), np.stack([ca, cb, ca]), v))
    return out


# ---- RANSAC --------------------------------------------------------------------------------------------------------------
class RansacCase(NamedTuple):
    name: str
    src: np.ndarray
    dst: np.ndarray
    corres: np.ndarray          # int32 [n_src]; entries outside [0, n_dst) are "no correspondence"
    ransac_n: int
    max_dist: float
    edge: float
    max_iter: int
    seed: int
    kind: str                   # "generic", "tie" (exact ties in count and rmse), "empty", "equality", "invalid"


def rigid(deg, axis, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = t
    return T


def _generic_set(rng, n, outliers):
    src = rng.uniform(-1.0, 1.0, (n, 3))
    Tg = rigid(25.0, [0.3, -0.2, 1.0], [0.4, 0.1, -0.3])
    dst = src @ Tg[:3, :3].T + Tg[:3, 3] + rng.normal(0, 0.005, src.shape)
    bad = rng.random(n) < outliers
    dst[bad] += rng.normal(0, 0.5, (int(bad.sum()), 3))
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return src, dst[perm], inv.astype(np.int32)


ITER_EDGES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2048)   # 256 threads, 4 hypotheses per block, 1 024 strided + tree
NSRC_EDGES = (1, 2, 3, 63, 64, 65)                                  # 64 scoring lanes


def ransac_cases():
    """Every case is built so that its winner is decided: either one hypothesis is best by a margin far above rounding, or
    the best ones tie exactly (the same bits on each side) and the earliest must win.  Hypotheses drawn from one sample set
    in another order tie only up to rounding, which no implementation can be held to; the tie cases avoid them by dyadic
    coordinates, for which the sums of the fit are exact in any order.  test_matching_cases_host.py checks all this."""
    out = []
    src, dst, corres = _generic_set(np.random.default_rng(2000), 200, 0.5)
    for it in ITER_EDGES:         # seed 15: the first hypothesis is valid for both sample sizes, so max_iter = 1 has a winner
        out.append(RansacCase(f"iter_{it}", src, dst, corres, 3 + it % 2, 0.075, 0.9, it, 15, "generic"))
    shift = np.array([1.5, -0.75, 2.0])
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    for n in NSRC_EDGES:
        for rn in (3, 4):
            if n == 1:      # every draw is the one pair: the same rank-0 fit (a translation), one exact inlier, rmse 0
                out.append(RansacCase(f"nsrc1_rn{rn}", tri[:1] + 0.5, tri[:1] + shift, np.zeros(1, np.int32), rn, 0.075, 0.9,
                                      2048 if rn == 3 else 1025, 3, "tie"))
            elif n <= 3:    # source edges of 1 against target edges of 4: a mixed draw fails the edge check, a pure one is
                            # a translation with itself as its one exact inlier: n of the n^rn distinct draws are valid
                            # and tie exactly
                for seed in ((0, 1, 2) if (n, rn) == (2, 3) else (0,)):
                    out.append(RansacCase(f"nsrc{n}_rn{rn}_s{seed}", tri[:n], 4.0 * tri[:n] + shift, np.arange(n, dtype=np.int32),
                                          rn, 0.075, 0.9, 2048, seed, "tie"))
            else:
                s, d, c = _generic_set(np.random.default_rng(2100 + n), n, 0.3)
                out.append(RansacCase(f"nsrc{n}_rn{rn}", s, d, c, rn, 0.075, 0.9, 1025, 40 + n, "generic"))
    # a valid hypothesis with no inlier.  Target edges are 8 times the source edges, so only a pure draw (one pair three
    # times) passes the edge check; its fit is a translation with residual exactly 0.  With max_corr_dist = 0 the distance
    # checker passes (0 > 0 is false) and scoring finds no inlier (0 < 0 is false): meta[2] > 0, yet nothing wins.
    s = 4.0 * tri
    out.append(RansacCase("valid_without_inlier", s, 8.0 * s + [1.0, 2.0, 3.0], np.arange(3, dtype=np.int32), 3, 0.0, 0.9, 257,
                          5, "empty"))
    # checker equality: two pairs on the x axis, source edge 5, target edge 4.5, ransac_n = 4 (mean = sum / 4 is exact).
    # Edge check: 4.5 < 5 * 0.9 is false in fp64 (the product rounds to 4.5), so a mixed draw passes AT equality.  Its fit
    # is rank 1 without a turn: a balanced draw {0, 0, 1, 1} leaves residuals of exactly 0.25 at both points, a draw
    # {0, 0, 0, 1} 0.125 and 0.375.
    #   edge_check_at_equality: max_corr_dist 0.3 -- balanced draws are valid with 2 inliers and win (earliest);
    #   distance_check_at_equality: max_corr_dist 0.25, edge_similarity 0.75 -- balanced draws pass the distance checker AT
    #   equality (0.25 > 0.25 is false) and have no inlier (0.25 < 0.25 is false); a pure draw wins with one.
    s = np.array([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0]])
    d = np.array([[10.0, 0.0, 0.0], [14.5, 0.0, 0.0]])
    out.append(RansacCase("edge_check_at_equality", s, d, np.arange(2, dtype=np.int32), 4, 0.3, 0.9, 256, 6, "equality"))
    out.append(RansacCase("distance_check_at_equality", s, d, np.arange(2, dtype=np.int32), 4, 0.25, 0.75, 256, 7, "equality"))
    # invalid correspondences: -1, n_dst and 2^31 - 1 at 10 % and at 100 % of the entries
    src, dst, corres = _generic_set(np.random.default_rng(2300), 200, 0.3)
    for frac in (10, 100):
        rng = np.random.default_rng(frac)
        c = corres.copy()
        hit = np.flatnonzero(rng.random(200) < frac / 100.0) if frac < 100 else np.arange(200)
        c[hit] = np.array([-1, len(dst), I32_MAX], np.int64)[np.arange(len(hit)) % 3].astype(np.int32)
        out.append(RansacCase(f"invalid_{frac}pct", src, dst, c, 3, 0.075, 0.9, 2048, 8, "invalid"))
        c4 = np.where((c >= 150) & (c <= 200), 150, c).astype(np.int32)        # a shorter target: more entries fall outside
        out.append(RansacCase(f"invalid_{frac}pct_rn4", src, dst[:150], c4, 4, 0.075, 0.9, 1025, 9, "invalid"))
    return out


def ransac_table(c):
    """Per hypothesis, as imf_oracle.ransac_registration scores them with the "no correspondence" rule: (picks [it, n],
    valid bool [it], inlier count [it] (-1 invalid), rmse [it], T [it, 4, 4], dis [it, n_src] (inf where there is no
    correspondence), checker residuals [it, ransac_n], edge lengths ds, dd [it, pairs])."""
    src, dst = np.asarray(c.src, np.float64), np.asarray(c.dst, np.float64)
    n = len(src)
    cor = np.asarray(c.corres, np.int64)
    has = (cor >= 0) & (cor < len(dst))
    cor = np.where(has, cor, 0)
    it = np.arange(c.max_iter, dtype=np.uint64)
    picks = np.stack([(O._splitmix64(np.uint64(c.seed) ^ (it * np.uint64(4) + np.uint64(j))) % np.uint64(n)).astype(np.int64)
                      for j in range(c.ransac_n)], 1)
    S, D = src[picks], dst[cor[picks]]
    ok = has[picks].all(1)
    ds_all, dd_all = [], []
    for i in range(c.ransac_n):
        for j in range(i + 1, c.ransac_n):
            ds = np.linalg.norm(S[:, i] - S[:, j], axis=1)
            dd = np.linalg.norm(D[:, i] - D[:, j], axis=1)
            ds_all.append(ds)
            dd_all.append(dd)
            ok &= ~((ds < dd * c.edge) | (dd < ds * c.edge))
    T = O.rigid_fit(S, D)
    moved = S @ np.swapaxes(T[:, :3, :3], 1, 2) + T[:, None, :3, 3]
    resid = np.linalg.norm(moved - D, axis=2)
    ok &= ~(resid > c.max_dist).any(1)
    tgt = dst[cor]
    dis = np.linalg.norm(src[None] @ np.swapaxes(T[:, :3, :3], 1, 2) + T[:, None, :3, 3] - tgt[None], axis=2)
    dis = np.where(has[None], dis, np.inf)
    inl = dis < c.max_dist
    count = np.where(ok, inl.sum(1), -1)
    rmse = np.sqrt(np.where(inl, dis * dis, 0.0).sum(1) / np.maximum(inl.sum(1), 1))
    return picks, ok, count, rmse, T, dis, resid, np.stack(ds_all, 1), np.stack(dd_all, 1)


def winner_count_longdouble(c, T):
    """The inlier count of the transform T over the valid correspondences with every distance in np.longdouble."""
    src, dst = np.asarray(c.src, np.longdouble), np.asarray(c.dst, np.longdouble)
    cor = np.asarray(c.corres, np.int64)
    has = (cor >= 0) & (cor < len(dst))
    T = np.asarray(T, np.longdouble)
    e = src[has] @ T[:3, :3].T + T[:3, 3] - dst[cor[has]]
    return int((np.sqrt((e * e).sum(1)) < np.longdouble(c.max_dist)).sum())


def end_to_end_case():
    """`run_ransac`'s call shape with one NaN descriptor row on each side: (xyz0, xyz1, feat0, feat1, voxel_size, Tg).
    feat0 rows are noisy copies of their target's descriptor; row 7 of feat0 and row 11 of feat1 hold a NaN."""
    rng = np.random.default_rng(31)
    src, dst, corres = _generic_set(rng, 300, 0.3)
    feat1 = unit_rows(rng, 300, 32)
    feat0 = (feat1[corres] + 0.01 * rng.standard_normal((300, 32))).astype(np.float32)
    feat0[7, 5] = np.nan
    feat1[11, 0] = np.nan
    return src, dst, feat0, feat1, 0.05
