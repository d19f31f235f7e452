"""Float64 NumPy restatement of the RGB-D odometry (csrc/odometry.hip, whose head states the rules): `prepare`, `stage`,
`odometry`, `track`.  Plain helper module: tests/test_odometry_host.py exercises it on the CPU, tests/test_gpu_odometry.py
runs the kernels against it.

Every per-pixel operation stands in the order the kernel's source has it, one rounding per operation, so the images of
`prepare`, the winner map and every addend of a stage can equal the kernel's bit for bit; only the order of the 29 sums
differs.  A stage also returns sum |addend| per sum (the scale of the summation error) and the margins of its decisions."""
import numpy as np

from plane_icp_restate import ldl_solve, update_from

LAMBDA, MAX_DEPTH_DIFF, MIN_CORR, ITERATIONS = 0.968, 0.03, 30, (20, 10, 5)


def intensity(color_u8):
    """(r + g + b) / 765: the integer sum first, then one division."""
    return color_u8.astype(np.int64).sum(-1).astype(np.float64) / 765.0


def smooth(I):
    """(1 2 1)/4 along the rows, then (1 2 1)/4 along the columns, the border replicated."""
    p = np.pad(I, ((0, 0), (1, 1)), mode="edge")
    h = ((p[:, :-2] + (p[:, 1:-1] + p[:, 1:-1])) + p[:, 2:]) / 4.0
    p = np.pad(h, ((1, 1), (0, 0)), mode="edge")
    return ((p[:-2] + (p[1:-1] + p[1:-1])) + p[2:]) / 4.0


def sobel(P):
    """(d/du, d/dv) with [-1 0 1; -2 0 2; -1 0 1] / 8 and its transpose at interior pixels, NaN on the border."""
    gx, gy = np.full(P.shape, np.nan), np.full(P.shape, np.nan)
    a, b, c = P[:-2, :-2], P[:-2, 1:-1], P[:-2, 2:]
    d, f = P[1:-1, :-2], P[1:-1, 2:]
    g, h, i = P[2:, :-2], P[2:, 1:-1], P[2:, 2:]
    gx[1:-1, 1:-1] = (((c - a) + ((f - d) + (f - d))) + (i - g)) / 8.0
    gy[1:-1, 1:-1] = (((g - a) + ((h - b) + (h - b))) + (i - c)) / 8.0
    return gx, gy


def depth_edge_mask(D, depth_edge):
    """(interior pixels whose nine depths are valid and within depth_edge of the centre, the smallest distance of a
    difference between two valid depths of a neighbourhood to depth_edge)."""
    ok = np.zeros(D.shape, bool)
    c = D[1:-1, 1:-1]
    good = np.ones(c.shape, bool)
    margin = np.inf
    H, W = D.shape
    with np.errstate(invalid="ignore"):
        for dv in (0, 1, 2):
            for du in (0, 1, 2):
                diff = np.abs(D[dv:H - 2 + dv, du:W - 2 + du] - c)
                good &= diff < depth_edge
                fin = np.isfinite(diff)
                if fin.any():
                    margin = min(margin, float(np.abs(diff[fin] - depth_edge).min()))
    ok[1:-1, 1:-1] = good
    return ok, margin


def prepare(depth_u16, color_u8, K, levels=3, depth_scale=1000.0, depth_min=0.0, depth_max=4.0, depth_edge=0.06):
    """The pyramid: a list of dict(Is, D, Isx, Isy, Dx, Dy, fx, fy, cx, cy), level 0 first, and `edge_margin`."""
    H, W = depth_u16.shape
    if not 1 <= levels <= 5 or H % (1 << (levels - 1)) or W % (1 << (levels - 1)) or min(H, W) >> (levels - 1) < 3:
        raise ValueError(f"{H} x {W} with {levels} levels")
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    d = depth_u16.astype(np.float64) / depth_scale
    D = np.where((depth_u16 > 0) & (depth_min < d) & (d < depth_max), d, np.nan)
    I = intensity(color_u8)
    out, margin = [], np.inf
    for l in range(levels):
        Is = smooth(I)
        Isx, Isy = sobel(Is)
        with np.errstate(invalid="ignore"):
            Dx, Dy = sobel(D)
        ok, m = depth_edge_mask(D, depth_edge)
        margin = min(margin, m)
        Dx, Dy = np.where(ok, Dx, np.nan), np.where(ok, Dy, np.nan)
        out.append(dict(Is=Is, D=D, Isx=Isx, Isy=Isy, Dx=Dx, Dy=Dy, fx=fx, fy=fy, cx=cx, cy=cy))
        if l + 1 < levels:
            I = ((Is[0::2, 0::2] + Is[0::2, 1::2]) + (Is[1::2, 0::2] + Is[1::2, 1::2])) / 4.0
            q = [D[0::2, 0::2], D[0::2, 1::2], D[1::2, 0::2], D[1::2, 1::2]]
            cnt = sum(np.isfinite(a).astype(np.float64) for a in q)
            a, b, c, e = (np.where(np.isfinite(t), t, 0.0) for t in q)
            with np.errstate(invalid="ignore", divide="ignore"):
                D = np.where(cnt > 0, ((a + b) + (c + e)) / cnt, np.nan)
            fx, fy, cx, cy = fx / 2.0, fy / 2.0, (cx - 0.5) / 2.0, (cy - 0.5) / 2.0
    return dict(levels=out, edge_margin=margin, shape=(H, W))


def rows(g0, g1, fx, fy, xp, yp, zp, own):
    """The Jacobian row [n, 6] of a gradient pair under the update [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5]."""
    iz = 1.0 / zp
    c0 = (g0 * fx) * iz
    c1 = (g1 * fy) * iz
    c2 = -((c0 * xp + c1 * yp) * iz) - own
    return np.stack([-(zp * c1) + yp * c2, zp * c0 - xp * c2, -(yp * c0) + xp * c1, c0, c1, c2], 1)


def stage(src, dst, level, T, max_depth_diff=MAX_DEPTH_DIFF, lam=LAMBDA, reverse=False):
    """One stage at one level with the source-to-target transformation T: dict(winner int32 [H_l, W_l] (source index or
    -1), sums [29] (n, cost, 21 upper entries of A, 6 of b), abs_sums [29], n_valid, margins dict(pixel, depth_diff,
    z_gap)).  reverse: the sums are taken in reversed winner order."""
    s, t = src["levels"][level], dst["levels"][level]
    H, W = s["D"].shape
    fx, fy, cx, cy = s["fx"], s["fy"], s["cx"], s["cy"]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = s["D"].ravel()
    valid = np.isfinite(d)
    idx = np.flatnonzero(valid)
    d = d[idx]
    x = ((u.ravel()[idx] - cx) * d) / fx
    y = ((v.ravel()[idx] - cy) * d) / fy
    xp = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * d) + T[0, 3]
    yp = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * d) + T[1, 3]
    zp = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * d) + T[2, 3]
    margins = dict(pixel=np.inf, depth_diff=np.inf, z_gap=np.inf)
    keep = zp > 0
    idx, xp, yp, zp = idx[keep], xp[keep], yp[keep], zp[keep]
    fx, fy, cx, cy = t["fx"], t["fy"], t["cx"], t["cy"]      # into the target through the target's intrinsics
    pu = ((fx * xp) / zp + cx) + 0.5
    pv = ((fy * yp) / zp + cy) + 0.5
    if len(pu):
        margins["pixel"] = float(min(np.abs(pu - np.rint(pu)).min(), np.abs(pv - np.rint(pv)).min()))
    keep = (pu >= 1.0) & (pu < W - 1.0) & (pv >= 1.0) & (pv < H - 1.0)         # 1 <= floor <= W - 2 (H - 2)
    idx, xp, yp, zp, pu, pv = idx[keep], xp[keep], yp[keep], zp[keep], pu[keep], pv[keep]
    ut, vt = np.floor(pu).astype(np.int64), np.floor(pv).astype(np.int64)
    tp = vt * W + ut
    Dt = t["D"].ravel()[tp]
    keep = np.isfinite(Dt) & np.isfinite(t["Dx"].ravel()[tp]) & np.isfinite(t["Dy"].ravel()[tp])
    idx, xp, yp, zp, tp, Dt = idx[keep], xp[keep], yp[keep], zp[keep], tp[keep], Dt[keep]
    diff = np.abs(Dt - zp)
    if len(diff):
        margins["depth_diff"] = float(np.abs(diff - max_depth_diff).min())
    keep = diff < max_depth_diff
    idx, xp, yp, zp, tp, Dt = idx[keep], xp[keep], yp[keep], zp[keep], tp[keep], Dt[keep]
    order = np.lexsort((idx, zp, tp))                       # by target pixel, then z', then source index
    first = np.ones(len(order), bool)
    first[1:] = tp[order][1:] != tp[order][:-1]
    second = np.flatnonzero(~first)
    second = second[first[second - 1]] if len(second) else second       # the runner-up of every contested pixel
    if len(second):
        gap = zp[order][second] - zp[order][second - 1]
        if (gap > 0).any():
            margins["z_gap"] = float(gap[gap > 0].min())
    win = order[first]
    win = win[np.argsort(idx[win])]                         # winners in source order
    idx, xp, yp, zp, tp, Dt = idx[win], xp[win], yp[win], zp[win], tp[win], Dt[win]
    winner = np.full(H * W, -1, np.int32)
    winner[tp] = idx
    rI = t["Is"].ravel()[tp] - s["Is"].ravel()[idx]
    rG = Dt - zp
    JI = rows(t["Isx"].ravel()[tp], t["Isy"].ravel()[tp], fx, fy, xp, yp, zp, 0.0)
    JG = rows(t["Dx"].ravel()[tp], t["Dy"].ravel()[tp], fx, fy, xp, yp, zp, 1.0)
    wg, wi = lam, 1.0 - lam
    add = np.empty((len(idx), 29))
    add[:, 0] = 1.0
    add[:, 1] = wg * (rG * rG) + wi * (rI * rI)
    k = 2
    for a in range(6):
        for b in range(a, 6):
            add[:, k] = wg * (JG[:, a] * JG[:, b]) + wi * (JI[:, a] * JI[:, b])
            k += 1
    for a in range(6):
        add[:, 23 + a] = wg * (JG[:, a] * rG) + wi * (JI[:, a] * rI)
    sums = (add[::-1] if reverse else add).sum(0) if len(add) else np.zeros(29)
    return dict(winner=winner.reshape(H, W), sums=sums, abs_sums=np.abs(add).sum(0), n_valid=int(valid.sum()),
                margins=margins)


def system(sums):
    """(n, cost, A [6, 6] exactly symmetric, b [6]) of a stage's 29 sums."""
    A = np.zeros((6, 6))
    k = 2
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = sums[k]
            k += 1
    return int(sums[0]), float(sums[1]), A, sums[23:29].copy()


def solve(sums, min_corr):
    """The update [4, 4] of a stage, or None under the singular rule or with fewer than min_corr winners."""
    n, _, A, b = system(sums)
    x = ldl_solve(A, -b) if n >= min_corr else None
    return None if x is None else update_from(x)


def odometry(src, dst, init=None, iterations=ITERATIONS, max_depth_diff=MAX_DEPTH_DIFF, lam=LAMBDA, min_corr=MIN_CORR,
             reverse=False):
    """(T [4, 4], info [6, 6], dict(n, fitness, cost, lost, flags, n_valid, winners: the winner map of every stage))."""
    levels = len(src["levels"])
    if len(iterations) != levels:
        raise ValueError(f"{len(iterations)} iteration counts for {levels} levels")
    T = np.eye(4) if init is None else np.array(init, np.float64)
    flags, winners = 0, []
    for k, its in enumerate(iterations):
        level = levels - 1 - k
        for _ in range(its):
            st = stage(src, dst, level, T, max_depth_diff, lam, reverse)
            winners.append(st["winner"])
            U = solve(st["sums"], min_corr)
            if U is None:
                flags |= 1
            else:
                T = U @ T
    st = stage(src, dst, 0, T, max_depth_diff, lam, reverse)
    winners.append(st["winner"])
    n, cost, A, _ = system(st["sums"])
    lost = solve(st["sums"], min_corr) is None
    flags |= 2 if lost else 0
    return T, A, dict(n=n, fitness=n / st["n_valid"] if st["n_valid"] else 0.0, cost=cost, lost=lost, flags=flags,
                      n_valid=st["n_valid"], winners=winners)


def track(depth, color, K, levels=3, iterations=ITERATIONS, max_depth_diff=MAX_DEPTH_DIFF, lam=LAMBDA, min_corr=MIN_CORR,
          **prep):
    """(poses cam2first [F, 4, 4], kept bool [F]): frame f against the last kept frame, from the identity; a lost pair drops
    frame f (NaN pose)."""
    frames = [prepare(depth[f], color[f], K, levels, **prep) for f in range(len(depth))]
    poses = np.full((len(depth), 4, 4), np.nan)
    kept = np.zeros(len(depth), bool)
    last = None
    for f in range(len(depth)):
        if last is None:
            poses[f], kept[f], last = np.eye(4), True, f
            continue
        T, _, res = odometry(frames[f], frames[last], None, iterations, max_depth_diff, lam, min_corr)
        if res["lost"]:
            continue
        poses[f], kept[f], last = poses[last] @ T, True, f
    return poses, kept


def pose_error(T, truth):
    """(rotation angle in degrees, translation distance in metres) between two rigid transformations."""
    R = T[:3, :3] @ truth[:3, :3].T
    return (float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))),
            float(np.linalg.norm(T[:3, 3] - truth[:3, 3])))


def pair_truth(poses, s, t):
    """Source camera s into target camera t, from cam2world poses."""
    return np.linalg.inv(poses[t]) @ poses[s]


# What this restatement gave on make_sequence(160, 120, n_frames=5, seed=0, holes=0.02, arc) with the colours of
# tsdf_color_scene (measured on a CPU with NumPy 2): the worst pair f -> f - 1 and the worst pose of
# `track` against the ground truth, (degrees, metres).  tests/test_odometry_host.py gates the restatement at twice these,
# tests/test_gpu_odometry.py the kernels' `track` at the same gate.
MEASURED = {
    0.12: dict(pair=(0.25263580394289475, 0.003566888467126352), track=(0.313879268511576, 0.003566888467126352)),
    0.3: dict(pair=(0.07609539066152463, 0.002880883716848013), track=(0.08152758461206072, 0.0037388088855450498)),
    0.5: dict(pair=(0.04752769049965299, 0.0020514575110387495), track=(0.04219986112883475, 0.0012501511493440817)),
}
# how far the final T of pair 1 -> 0 at arc 0.12 moved between NumPy's sums and the reversed pixel order, same machine
DELTA_MEASURED = 6.088879400678593e-16


def sequence(arc, n_frames=5, seed=0):
    """The synthetic sequence the odometry tests share, with its colours."""
    import tsdf_color_scene as CS
    import tsdf_scene as S
    seq = S.make_sequence(160, 120, n_frames=n_frames, seed=seed, holes=0.02, arc=arc)
    seq["color"] = CS.make_colors(seq)
    return seq


def order_sensitivity(arc=0.12, **prep):
    """(forward, reversed, delta, delta_info): `odometry` on pair 1 -> 0 with NumPy's sums and with the sums in reversed
    pixel order, the largest element difference of the two T, and of the two info relative to info's largest entry."""
    seq = sequence(arc)
    src, dst = (prepare(seq["depth"][f], seq["color"][f], seq["K"], **prep) for f in (1, 0))
    fwd, rev = odometry(src, dst), odometry(src, dst, reverse=True)
    return fwd, rev, float(np.abs(fwd[0] - rev[0]).max()), float(np.abs(fwd[1] - rev[1]).max() / np.abs(fwd[1]).max())
