"""The catalogue of adversarial frames and cameras for imf_tsdf_allocate / imf_tsdf_integrate(_rgb) (csrc/tsdf.hip), CPU only:
the inputs of tests/test_gpu_tsdf_exact.py, the rule its state comparisons obey, and the self-checks that
tests/test_tsdf_cases_host.py runs without a GPU (every case really reaches what it was built to reach).

  A  frame counts: 64 units around the origin, up to 257 frames in one call, cameras turning through many full turns, so
     that every 32-bit word of the kernel's frame mask and every trip of its fill loop carries frames that matter
  B  the frustum cull: a dense 6 x 6 x 6 block with the eye inside, rolled and tilted cameras, a principal point outside the
     image, fx about 2 fy; every one of the six cull conditions cuts through units the frame updates
  C  the per-voxel thresholds at equality, in power-of-two arithmetic that fp64 carries exactly
  D  allocate: image sides that are no multiple of the stride, depth at un-sampled pixels only, points exactly on unit
     boundaries, reach 3 and 4, the first and the last permitted unit coordinate

The yardstick is the un-culled NumPy restatement (tsdf_restate.py, tsdf_color_restate.py) plus literal expected values."""
import concurrent.futures as cf
import math

import numpy as np

import tsdf_color_restate as CR
import tsdf_restate as R

RES = R.RES
# A frame that is culled or masked out by mistake removes every voxel it updates in the unit: at least 64 for the (unit,
# frame) pairs the self-checks count.  A projection within rounding of a threshold moves single voxels.
UNIT_CAP = 4
COORD_LIM = 1 << 17                                          # unit coordinates lie in [-2^17, 2^17) (csrc/common.h)
RIGID_TOL = 5e-7                                             # imfnet_amd/fuse.py: RIGID_TOL


def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    S = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * S + (1.0 - math.cos(angle)) * (S @ S)


def pose(eye, rot):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot, eye
    return T


def intrinsic(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def block(lo, hi):
    """All units with coordinates lo .. hi per axis, int32 [n, 3] = (x, y, z), ascending in (z, y, x)."""
    r = np.arange(lo, hi + 1)
    z, y, x = np.meshgrid(r, r, r, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)


def world2cam(poses_cam2world):
    """As TSDFVolume.integrate forms it: the inverse of every finite pose, a NaN matrix for every other one."""
    P = np.asarray(poses_cam2world, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([np.linalg.inv(T) if np.isfinite(T).all() else np.full((4, 4), np.nan) for T in P])


def rigid_error(mats):
    """Worst |singular value - 1| of the rotation blocks of the finite matrices."""
    M = np.asarray(mats, np.float64)
    M = M[np.isfinite(M).all((1, 2))]
    return float(np.abs(np.linalg.svd(M[:, :3, :3], compute_uv=False) - 1.0).max())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def state_differences(got, ref):
    """got, ref = (tsdf, w[, colour]) as [n, 16, 16, 16(, 3)] float32.  Counts by bits: voxels with w != 0 in ref, voxels
    whose (tsdf, w) differ, the most of them in one unit, and voxels whose (tsdf, w) agree but whose colour does not."""
    n = len(ref[0])
    differ = (_bits(got[0]) != _bits(ref[0])) | (_bits(got[1]) != _bits(ref[1]))
    per_unit = differ.reshape(n, -1).sum(1)
    colour = 0
    if len(ref) > 2:
        colour = int(((_bits(got[2]) != _bits(ref[2])).any(-1) & ~differ).sum())
    return dict(seen=int((ref[1] != 0).sum()), differ=int(differ.sum()), worst_unit=int(per_unit.max()) if n else 0,
                colour=colour)


def assert_state_rule(d, cap):
    """The comparison rule of the cases A, B and D; `cap` is STATE_CAP of test_tsdf_color_host.py."""
    assert d["seen"] > 0
    assert d["differ"] <= cap * d["seen"], d
    assert d["worst_unit"] <= UNIT_CAP, d
    assert d["colour"] == 0, d


# ---- A: frame counts ---------------------------------------------------------------------------------------------------
A_FRAMES = (32, 33, 65, 257)
A_OFFSETS = (0.5, 0.0)
A_W, A_H = 32, 24


def case_a(lattice_offset):
    """257 frames; a test of F frames takes the first F.  Every 17th pose (16, 33, 50, ...) is NaN."""
    F = max(A_FRAMES)
    rng = np.random.default_rng(11)
    K = intrinsic(21.0, 17.0, 0.3 * A_W, 0.7 * A_H)
    p = R.params(voxel_length=0.01, sdf_trunc=0.04, depth_trunc=0.5, lattice_offset=lattice_offset)
    roll = rotation([0.0, 0.0, 1.0], 0.6)
    poses = np.empty((F, 4, 4))
    for f in range(F):
        eye = 0.03 * np.array([math.cos(0.7 * f), math.sin(0.9 * f), math.cos(0.4 * f + 1.0)])
        nod = rotation([1.0, 0.0, 0.0], 0.9 * math.sin(0.11 * f))             # the optical axis leaves the turn's plane
        poses[f] = pose(eye, rotation([0.3, 1.0, 0.2], 0.37 * f) @ nod @ roll)      # 257 frames: 15 full turns
    poses[16::17] = np.nan
    v, u = np.meshgrid(np.arange(A_H), np.arange(A_W), indexing="ij")
    depth = np.empty((F, A_H, A_W), np.uint16)
    for f in range(F):
        depth[f] = np.rint(420.0 + 20.0 * np.sin(0.4 * u + 0.3 * f) * np.cos(0.3 * v - 0.2 * f)).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.05] = 0
    color = rng.integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    return dict(units=block(-2, 1), depth=depth, color=color, poses=poses, K=K, p=p, height=A_H, width=A_W)


def restate_a(case, fused=False):
    """{F: (tsdf, w, colour)} for F in A_FRAMES from one walk over the 257 frames, and the trace of that walk.  The units
    are independent of each other, so four threads walk a quarter of them each."""
    w2c = world2cam(case["poses"])

    def walk(rows):
        out, state, trace, a = {}, None, [], 0
        for F in A_FRAMES:
            state = CR.integrate_rgb(case["units"][rows], case["depth"][a:F], case["color"][a:F], w2c[a:F], case["K"],
                                     case["p"], state=state, fused=fused, trace=trace)
            out[F], a = state, F
        return out, np.stack(trace)

    with cf.ThreadPoolExecutor(4) as pool:
        parts = list(pool.map(walk, np.array_split(np.arange(len(case["units"])), 4)))
    states = {F: tuple(np.concatenate([part[0][F][k] for part in parts]) for k in range(3)) for F in A_FRAMES}
    return states, np.concatenate([part[1] for part in parts], 1)      # trace [257, n]: voxels updated per frame and unit


def check_a(case, states, trace):
    """The self-checks of case A on the restatement's own walk."""
    for F in A_FRAMES:
        t = trace[:F]
        for g in range(0, F, 32):                            # every word of the frame mask, the last partial one too
            assert ((t[g:min(g + 32, F)] >= 64).sum(1) >= 8).any(), (F, g)      # 8 units with 64 voxels each
        assert (t[F - 1] > 0).any(), F
        assert ((t > 0).sum(1) == 0).any(), F
        assert states[F][1].max() >= 6.0, F
    nan = ~np.isfinite(case["poses"]).all((1, 2))
    assert nan[16] and nan.sum() == 15 and (trace[nan] == 0).all()
    # every unit is seen by several separate runs of frames
    seen = trace > 0
    runs = (seen[1:] & ~seen[:-1]).sum(0) + seen[0]
    assert runs.min() >= 3, runs.min()


# ---- B: the cull -------------------------------------------------------------------------------------------------------
B_W, B_H = 32, 24
B_RAW = 295                                                  # a constant plane just under depth_trunc
# (eye, rotation axis, angle, (fx, fy, cx, cy)): rolled and tilted, the eye inside the block (|coordinate| < 0.288 m)
# 1: the principal point left of the image (cx < 0); 2: fx about 2 fy; 5: the principal point below the image (cy > H).
# Chosen among seeded random candidates for the count of mixed (unit, frame) pairs; the host test asserts what they deliver.
B_CAMERAS = (
    ((-0.044, 0.119, -0.048), (-0.86, 0.9, -1.3), 2.78, (20.0, 22.0, 15.5, 11.5)),
    ((-0.119, -0.18, -0.113), (0.62, 0.13, 0.71), 1.28, (18.0, 19.0, -6.0, 9.0)),
    ((-0.071, 0.05, 0.003), (2.77, -0.19, 1.27), 1.56, (40.0, 20.5, 12.3, 14.1)),
    ((-0.124, -0.067, -0.03), (-0.05, 0.49, -0.31), 1.21, (15.0, 13.0, 22.4, 5.2)),
    ((-0.15, -0.059, -0.07), (-1.01, 0.37, 1.59), 2.37, (26.0, 24.0, 9.6, 16.8)),
    ((-0.131, 0.134, -0.057), (0.75, 0.67, -1.06), 0.88, (17.0, 21.0, 20.0, 30.0)),
)


def b_params():
    return R.params(voxel_length=0.006, sdf_trunc=0.04, depth_trunc=0.3, lattice_offset=0.5)


def case_b(cameras=B_CAMERAS):
    """Single-frame calls, each with its own intrinsics, onto one state."""
    rng = np.random.default_rng(12)
    poses = np.stack([pose(np.array(e), rotation(ax, ang)) for e, ax, ang, _ in cameras])
    Ks = [intrinsic(*k) for _, _, _, k in cameras]
    depth = np.full((len(cameras), B_H, B_W), B_RAW, np.uint16)
    color = rng.integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    return dict(units=block(-3, 2), depth=depth, color=color, poses=poses, Ks=Ks, p=b_params(), height=B_H, width=B_W)


def case_b_float32():
    """Case B's cameras as the fragment command line would hand them over: the poses under a world transform, rounded to
    float32, made relative to the first one in float32 (fuse_fragments.select_frames), widened.  The volume is then the
    first camera's frame."""
    case = case_b()
    world = pose(np.array([1.7, -2.9, 0.6]), rotation([0.2, -0.5, 0.8], 2.1))
    raw = [(world @ T).astype(np.float32) for T in case["poses"]]
    base_inv = np.linalg.inv(raw[0])
    rel = np.stack([np.matmul(base_inv, T) for T in raw])
    assert rel.dtype == np.float32
    case["poses"] = rel.astype(np.float64)
    return case


def restate_b(case, fused=False, trace=None):
    w2c = world2cam(case["poses"])
    state = None
    for f, K in enumerate(case["Ks"]):
        state = CR.integrate_rgb(case["units"], case["depth"][f:f + 1], case["color"][f:f + 1], w2c[f:f + 1], K, case["p"],
                                 state=state, fused=fused, trace=trace)
    return state


def mixed_pairs(case, trace):
    """{condition: number of (unit, frame) pairs in which some voxels of the unit pass the condition and some fail it,
    and the frame updates at least 64 voxels of the unit}.  The image sides are judged among the voxels in front of the
    camera."""
    w2c = world2cam(case["poses"])
    count = dict.fromkeys(R.CULL_CONDITIONS, 0)
    n = len(case["units"])
    for f, K in enumerate(case["Ks"]):
        c = R.cull_conditions(case["units"], w2c[f], K, case["p"], case["height"], case["width"])
        front = c["front"].reshape(n, -1)
        for name in R.CULL_CONDITIONS:
            ok = c[name].reshape(n, -1)
            among = np.ones_like(front) if name in ("front", "near") else front
            mixed = (ok & among).any(1) & (~ok & among).any(1)
            count[name] += int((mixed & (trace[f] >= 64)).sum())
    return count


B_CORNER_SLACK = 0.06                                        # voxels; 1 % of the bounding sphere's radius is 0.13


def case_b_corner(name):
    """One unit that the frame sees by a single corner voxel: the plane of the cull condition `name` stands square to the
    unit's diagonal and passes 0.06 voxels inside the corner sample, so the corner voxel is in (by 1e-4 m, no rounding
    question), the next ones are 0.58 voxels further out, and the unit's bounding sphere reaches past the plane by 0.5 % of
    its radius only.  A cull with a sphere that is too small by that much drops the voxel."""
    p = R.params(voxel_length=0.006, sdf_trunc=0.04, depth_trunc=0.25, lattice_offset=0.5)
    K = intrinsic(20.0, 22.0, 15.0, 11.0)
    width, height, vl = 32, 24, p["voxel_length"]
    eps = B_CORNER_SLACK * vl
    ax0, ax1 = (-K[0, 2] - 0.5) / K[0, 0], (width - K[0, 2] - 0.5) / K[0, 0]
    ay0, ay1 = (-K[1, 2] - 0.5) / K[1, 1], (height - K[1, 2] - 0.5) / K[1, 1]
    h = lambda a: math.sqrt(1.0 + a * a)
    # the inward normal of the plane in the camera's frame, and the corner voxel's camera coordinates: eps inside
    n_c, p_c = {"front": ((0.0, 0.0, 1.0), (0.0, 0.0, eps)),
                "near": ((0.0, 0.0, -1.0), (0.0, 0.0, p["depth_trunc"] + p["sdf_trunc"] - eps)),
                "left": ((1.0 / h(ax0), 0.0, -ax0 / h(ax0)), (0.1 * ax0 + eps * h(ax0), 0.0, 0.1)),
                "right": ((-1.0 / h(ax1), 0.0, ax1 / h(ax1)), (0.1 * ax1 - eps * h(ax1), 0.0, 0.1)),
                "top": ((0.0, 1.0 / h(ay0), -ay0 / h(ay0)), (0.0, 0.1 * ay0 + eps * h(ay0), 0.1)),
                "bottom": ((0.0, -1.0 / h(ay1), ay1 / h(ay1)), (0.0, 0.1 * ay1 - eps * h(ay1), 0.1))}[name]
    n_c, p_c = np.array(n_c), np.array(p_c)
    unit, sign = np.array([1, -2, 0]), np.array([1.0, -1.0, 1.0])
    local = np.where(sign > 0, RES - 1, 0)
    corner = ((RES * unit + local).astype(np.float64) + p["lattice_offset"]) * vl
    g = sign / math.sqrt(3.0)                                 # the diagonal towards that corner, in the volume's frame
    axis = np.cross(g, n_c)                                   # world2cam's rotation takes g to n_c, then rolls about n_c
    rot = rotation(n_c, 0.8) @ rotation(axis, math.atan2(np.linalg.norm(axis), g @ n_c))
    assert np.abs(rot @ g - n_c).max() < 1e-12
    w2c = pose(p_c - rot @ corner, rot)
    depth = np.full((1, height, width), 250, np.uint16)
    color = np.random.default_rng(14).integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    return dict(units=unit[None].astype(np.int32), depth=depth, color=color, poses=np.linalg.inv(w2c)[None], K=K, p=p,
                height=height, width=width, corner=tuple(local[::-1].tolist()), normal=g)


# ---- C: exact thresholds -----------------------------------------------------------------------------------------------
C_W, C_H = 32, 24
C_VL, C_TRUNC = 2.0 ** -7, 2.0 ** -5
C_COLOUR = (200, 0, 255)


def c_units():
    """x, y in {-1, 0}, z in {0, 1, 2}: the global voxels (i, j, k) with -16 <= i, j < 16 and 0 <= k < 48."""
    r = np.array([-1, 0])
    z, y, x = np.meshgrid(np.arange(3), r, r, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)


def c_voxel(state_array, units, g):
    """The value at the global voxel g = (i, j, k) of a state array [n, 16, 16, 16, ...]."""
    g = np.asarray(g)
    row = {tuple(c): i for i, c in enumerate(np.asarray(units).tolist())}[tuple((g >> 4).tolist())]
    l = g & 15
    return state_array[row, l[2], l[1], l[0]]


def c_quantities(g, K, p, raw, width, height):
    """The rule's fp64 quantities at the global voxel g under the identity pose, in the rule's order of operations; the
    ones behind a skip are None."""
    x, y, z = (float(i) * p["voxel_length"] for i in g)     # lattice_offset 0
    q = dict(z=z, uf=None, vf=None, d=None, sdf=None)
    if not z > 0.0:
        return q
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    q["uf"], q["vf"] = fx * x / z + cx + 0.5, fy * y / z + cy + 0.5
    if not (0.0 <= q["uf"] < width and 0.0 <= q["vf"] < height):
        return q
    iu, iv = int(q["uf"]), int(q["vf"])
    q["d"] = float(np.float32(raw) / np.float32(p["depth_scale"]))
    a, b = (iu - cx) / fx, (iv - cy) / fy
    q["sdf"] = (q["d"] - z) * math.sqrt(a * a + b * b + 1.0)
    return q


def _case_c(K, raw, depth_trunc):
    p = R.params(voxel_length=C_VL, sdf_trunc=C_TRUNC, depth_scale=1000.0, depth_trunc=depth_trunc, lattice_offset=0.0)
    depth = np.full((1, C_H, C_W), raw, np.uint16)
    color = np.broadcast_to(np.array(C_COLOUR, np.uint8), depth.shape + (3,)).copy()
    return dict(units=c_units(), depth=depth, color=color, poses=np.eye(4)[None], K=K, p=p, height=C_H, width=C_W, raw=raw)


def case_c1():
    """cx = cy = -0.5, fx = 4 W, fy = 4 H: uf = fx x / z, vf = fy y / z.  Raw depth 250 = depth_trunc."""
    case = _case_c(intrinsic(4.0 * C_W, 4.0 * C_H, -0.5, -0.5), 250, 0.25)
    case["expect"] = {(0, 0, 16): (1.0, 1.0), (3, 0, 16): (1.0, 1.0), (0, 0, 28): (1.0, 1.0),
                      (4, 0, 16): (0.0, 0.0), (0, 4, 16): (0.0, 0.0), (0, 0, 0): (0.0, 0.0)}
    q = lambda g: c_quantities(g, case["K"], case["p"], 250, C_W, C_H)
    assert q((0, 0, 16))["uf"] == 0.0 and q((0, 0, 16))["vf"] == 0.0             # uf == 0: in
    assert q((3, 0, 16))["uf"] == 0.75 * C_W
    assert q((4, 0, 16))["uf"] == float(C_W) and q((4, 0, 16))["vf"] == 0.0      # uf == W: out
    assert q((0, 4, 16))["vf"] == float(C_H) and q((0, 4, 16))["uf"] == 0.0      # vf == H: out
    assert q((0, 0, 0))["z"] == 0.0                                               # z == 0: out
    assert q((0, 0, 16))["d"] == case["p"]["depth_trunc"] == 0.25                # d == depth_trunc: in
    assert q((0, 0, 28))["d"] - q((0, 0, 28))["z"] == C_TRUNC and q((0, 0, 28))["sdf"] > C_TRUNC
    return case


def case_c2():
    """Integer cx, cy: the pixel under the voxels (0, 0, k) has a = b = 0, so sdf = d - z exactly."""
    case = _case_c(intrinsic(64.0, 64.0, 16.0, 12.0), 250, 0.25)
    case["expect"] = {(0, 0, 36): (0.0, 0.0), (0, 0, 35): (-0.75, 1.0), (0, 0, 32): (0.0, 1.0), (0, 0, 28): (1.0, 1.0),
                      (0, 0, 27): (1.0, 1.0), (0, 0, 0): (0.0, 0.0)}
    q = lambda g: c_quantities(g, case["K"], case["p"], 250, C_W, C_H)
    assert q((0, 0, 36))["sdf"] == -C_TRUNC                                       # sdf == -sdf_trunc: out
    assert q((0, 0, 35))["sdf"] / C_TRUNC == -0.75
    assert q((0, 0, 32))["sdf"] == 0.0 and q((0, 0, 32))["z"] == q((0, 0, 32))["d"]
    assert q((0, 0, 28))["sdf"] == C_TRUNC                                        # sdf == sdf_trunc: 1 by either branch
    assert q((0, 0, 27))["sdf"] > C_TRUNC
    return case


def case_c_trunc(raw):
    """depth_trunc = 0.5 m against raw 500 (d == depth_trunc: a measurement), 501 (none) and 0 (none)."""
    case = _case_c(intrinsic(64.0, 64.0, 16.0, 12.0), raw, 0.5)
    d = float(np.float32(raw) / np.float32(1000.0))
    assert {500: d == 0.5, 501: d > 0.5, 0: d == 0.0}[raw]
    case["expect"] = {(0, 0, 16): (1.0, 1.0) if raw == 500 else (0.0, 0.0)}
    case["updates"] = raw == 500
    return case


# ---- D: allocate -------------------------------------------------------------------------------------------------------
D_SIZES = ((30, 22), (33, 25))                               # (width, height): neither side a multiple of the stride 4


def _d_depth(rng, F, height, width):
    depth = rng.integers(120, 300, (F, height, width)).astype(np.uint16)        # 0.12 .. 0.3 m: all within depth_trunc
    depth[rng.random(depth.shape) < 0.1] = 0
    return depth


def cases_d_cameras():
    """Case B's cameras (negative unit coordinates), one volume per intrinsics and image size, all poses in one call."""
    b = case_b()
    rng = np.random.default_rng(13)
    out = []
    for width, height in D_SIZES:
        for K in b["Ks"][:3]:
            out.append(dict(name=f"cameras {width}x{height} fx={K[0, 0]:g} cx={K[0, 2]:g}", K=K, height=height, width=width,
                            p=b["p"], depth=_d_depth(rng, len(b["poses"]), height, width), poses=b["poses"]))
    return out


def cases_d_sampling():
    """Valid depth only where the stride-4 sampling never looks (no unit), and only in the last sampled column and row."""
    b = case_b()
    out = []
    for width, height in D_SIZES:
        v, u = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
        sampled = (u % 4 == 0) & (v % 4 == 0)
        last = sampled & ((u == (width - 1) // 4 * 4) | (v == (height - 1) // 4 * 4))
        for name, mask in (("unsampled", ~sampled), ("last", last)):
            depth = np.where(mask, 200 + (u + 3 * v) % 90, 0).astype(np.uint16)[None].repeat(len(b["poses"]), 0)
            out.append(dict(name=f"{name} {width}x{height}", K=b["Ks"][0], height=height, width=width, p=b["p"], depth=depth,
                            poses=b["poses"], empty=name == "unsampled"))
    return out


def _pow2_frame(translation):
    """16 x 12, fx = fy = 8, cx = 8, cy = 4, raw 250: the samples u = 0, 4, 8, 12 and v = 0, 4, 8 back-project to
    x = (u - 8) / 32, y = (v - 4) / 32, z = 1 / 4 -- multiples of the unit length 1 / 8, -1 unit length among them."""
    p = R.params(voxel_length=C_VL, sdf_trunc=C_TRUNC, depth_trunc=6.0, lattice_offset=0.0)
    return dict(K=intrinsic(8.0, 8.0, 8.0, 4.0), height=12, width=16, p=p, depth=np.full((1, 12, 16), 250, np.uint16),
                poses=pose(np.asarray(translation, np.float64), np.eye(3))[None])


def case_d_boundaries():
    """Every sample exactly on a unit boundary in all three coordinates: floor must not round."""
    case = _pow2_frame((0.0, 0.0, -0.375))
    ul = RES * C_VL
    q = np.array([[(u - 8.0) * 0.25 / 8.0 / ul, (v - 4.0) * 0.25 / 8.0 / ul, (0.25 - 0.375) / ul]
                  for v in (0, 4, 8) for u in (0, 4, 8, 12)])
    assert (q == np.round(q)).all() and q[:, 0].min() == -2.0 and (q[:, 0] == -1.0).any() and (q[:, 2] == -1.0).all()
    found = {tuple((c + np.array(d)).tolist()) for c in q.astype(np.int64) for d in np.ndindex(3, 3, 3)}
    case["expect"] = np.array(sorted(found, key=lambda c: (c[2], c[1], c[0])), np.int32) - 1       # reach 1
    return case


def cases_d_reach():
    """voxel_length 0.001: sdf_trunc 0.04 reaches 3 units, 0.064 reaches 4 (the most), 0.07 would reach 5.  A 4 x 4 image
    has one sample."""
    out = []
    for trunc, reach in ((0.04, 3), (0.064, 4), (0.07, 5)):
        p = R.params(voxel_length=0.001, sdf_trunc=trunc, depth_trunc=6.0, lattice_offset=0.5)
        assert int(math.ceil(trunc / (RES * 0.001))) == reach
        out.append(dict(K=intrinsic(5.0, 5.0, 1.5, 1.5), height=4, width=4, p=p, depth=np.full((1, 4, 4), 300, np.uint16),
                        poses=pose(np.array([0.003, -0.002, 0.001]), rotation([1.0, 2.0, 3.0], 0.4))[None], reach=reach,
                        n_units=(2 * reach + 1) ** 3))
    return out


def cases_d_range():
    """A frame pushed along one axis until the unit coordinate of its largest (smallest) sample is the last (first)
    permitted one, 2^17 - 2 - reach (-(2^17 - 1 - reach)), and one unit further; behind it a frame at the origin, which
    must open its units either way.  The pushed frame's x samples span the units -2 .. 1, y -1 .. 1, z is unit 2."""
    ul, reach = RES * C_VL, 1
    last, first = COORD_LIM - 2 - reach, -(COORD_LIM - 1 - reach)
    out = []
    for axis in range(3):
        hi, lo = ((1, -2), (1, -1), (2, 2))[axis]
        for name, shift, in_range in (("last", last - hi, True), ("past the last", last - hi + 1, False),
                                      ("first", first - lo, True), ("before the first", first - lo - 1, False)):
            t = np.zeros(3)
            t[axis] = shift * ul
            assert t[axis] / ul == shift
            far, near = _pow2_frame(t), _pow2_frame((0.0, 0.0, 0.0))
            case = dict(near, name=f"axis {axis} {name}", depth=np.concatenate([far["depth"], near["depth"]]),
                        poses=np.concatenate([far["poses"], near["poses"]]), in_range=in_range, axis=axis)
            # what the restatement (which knows no range) opens for the samples that are in range
            depth = case["depth"].copy()
            if not in_range:                                 # the samples of the pushed frame beyond the limit open nothing
                u = np.arange(16)
                v = np.arange(12)
                q = ((u - 8.0) / 32.0 / ul, (v - 4.0) / 32.0 / ul, np.array([2.0]))[axis] + shift
                bad = (q > last) | (q < first)
                if axis == 0:
                    depth[0][:, bad] = 0
                elif axis == 1:
                    depth[0][bad, :] = 0
                else:
                    depth[0][:] = 0
            case["expect"] = R.allocate(depth, case["poses"], case["K"], case["p"])
            case["extreme"] = last + reach if shift > 0 else first - reach
            out.append(case)
    return out
