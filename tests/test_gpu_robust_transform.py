"""imf_robust_transform (matching.robust_transform) on the GPU: every case of tests/golden/robust_transform.npz against
upstream's recorded float32 result, within 4 x the float32-vs-fp64 gap the generator stored for the case's family;
bit-identical repeats; the unsolvable systems; a set far past the register-resident share."""
import numpy as np
import pytest
import torch

import robust_restate as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cases():
    return RR.load_cases()


def _gaps(T, T_ref):
    T_ref = np.asarray(T_ref, np.float64)
    return np.abs(T[:3, :3] - T_ref[:3, :3]).max(), np.abs(T[:3, 3] - T_ref[:3, 3]).max()


def test_every_fixture_case_within_upstreams_own_float32_gap(cases):
    from imfnet_amd.matching import robust_transform
    for fam, seed, p0, p1, w, T_up, gap_R, gap_t in cases:
        tol_R, tol_t = RR.family_tolerance(cases, fam)
        T, ok = robust_transform(p0, p1, w, device=DEV)
        dR, dt = _gaps(T, T_up)
        rR, rt = _gaps(T, RR.robust_transform_f64(p0, p1, w))            # printed, not gated
        print(f"{fam} seed {seed}: vs upstream |dR| {dR:.2e} (tol {tol_R:.2e}) |dt| {dt:.2e} (tol {tol_t:.2e}); "
              f"vs fp64 restatement |dR| {rR:.2e} |dt| {rt:.2e}")
        assert ok, (fam, seed)
        assert T.dtype == np.float64 and T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1])
        assert dR <= tol_R and dt <= tol_t, (fam, seed, dR, tol_R, dt, tol_t)


def test_two_calls_are_bit_identical_and_none_is_ones(cases):
    from imfnet_amd.matching import robust_transform
    for fam, seed, p0, p1, w, *_ in cases[::3]:
        a, ok_a = robust_transform(p0, p1, w, device=DEV)
        b, ok_b = robust_transform(p0, p1, w, device=DEV)
        assert ok_a and ok_b and a.tobytes() == b.tobytes(), (fam, seed)
        if w is None:
            c, ok_c = robust_transform(p0, p1, np.ones(len(p0)), device=DEV)
            assert ok_c and a.tobytes() == c.tobytes(), (fam, seed)
    # device tensors in: the same bits as host arrays in
    fam, seed, p0, p1, w, *_ = cases[0]
    a, _ = robust_transform(p0, p1, None, device=DEV)
    d, _ = robust_transform(torch.as_tensor(p0).double().to(DEV), torch.as_tensor(p1).to(DEV), None, device=DEV)
    assert a.tobytes() == d.tobytes()


def test_unsolvable_systems_are_flagged_not_faults(cases):
    from imfnet_amd.matching import robust_transform
    g = np.random.default_rng(0)
    line = np.outer(np.arange(3.0) + 1.0, [1.0, 2.0, -0.5]) + [0.3, 0.1, 0.2]
    bad = {
        "n=1": (g.random((1, 3)), g.random((1, 3))),
        "n=2": (g.random((2, 3)), g.random((2, 3))),
        "3 collinear": (line, line + [0.1, 0.0, 0.0]),
        "40 collinear": (np.outer(np.linspace(-2, 2, 40), [0.5, -1.0, 2.0]),) * 2,
    }
    fam, seed, p0, p1, *_ = cases[0]
    nan0 = p0.astype(np.float64).copy()
    nan0[1234, 1] = np.nan
    bad["a NaN row in pts0"] = (nan0, p1)
    nan1 = p1.astype(np.float64).copy()
    nan1[4999, 2] = np.nan
    bad["a NaN row in pts1"] = (p0, nan1)
    for name, (a, b) in bad.items():
        T, ok = robust_transform(a, b, device=DEV)
        assert not ok and np.array_equal(T, np.eye(4)), name
    T, ok = robust_transform(p0, p1, np.zeros(len(p0)), device=DEV)        # no usable row at all
    assert not ok and np.array_equal(T, np.eye(4))
    # three rows that do span: solvable, and exact for an exact rigid motion
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]])
    R = RR.rotation([0.2, -1.0, 0.4], 6.0)
    T, ok = robust_transform(tri, tri @ R.T + [0.1, -0.2, 0.05], device=DEV)
    assert ok and np.abs(T[:3, :3] - R).max() < 1e-9 and np.abs(T[:3, 3] - [0.1, -0.2, 0.05]).max() < 1e-9
    # the library still answers afterwards
    T, ok = robust_transform(p0, p1, device=DEV)
    assert ok


def test_empty_set_launches_nothing_and_is_flagged():
    from imfnet_amd import _lib
    from imfnet_amd.matching import robust_transform
    T, ok = robust_transform(np.zeros((0, 3)), np.zeros((0, 3)), device=DEV)
    assert not ok and np.array_equal(T, np.eye(4))
    L = _lib.lib()
    out = torch.full((17,), -3.0, dtype=torch.float64, device=DEV)
    rc = L.imf_robust_transform(None, None, None, 0, out.data_ptr(), out[16:].data_ptr(), None, 0,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(out[:16].cpu().numpy().reshape(4, 4), np.eye(4))
    assert int(out[16:].view(torch.int32)[0]) == 1
    # a missing workspace for a set that needs one is an error code, not a launch
    n = 6000
    p = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
    assert L.imf_robust_transform_workspace_bytes(n) > 0
    rc = L.imf_robust_transform(p.data_ptr(), p.data_ptr(), None, n, out.data_ptr(), out[16:].data_ptr(), None, 0,
                                torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"workspace" in L.imf_last_error()


@pytest.mark.parametrize("n", [5120, 5121, 70000])
def test_sets_past_the_register_share(cases, n):
    """n = 5120 is the last register-resident size, 5121 the first that lives in the workspace, 70 000 far past it: each
    against the fp64 restatement of a freshly generated outdoor case, within the outdoor family's tolerance."""
    from imfnet_amd.matching import robust_transform
    kw = dict(RR.FAMILIES["outdoor_5deg"], n=n)
    p0, p1, w, planted = RR.make_case(seed=7, **kw)
    tol_R, tol_t = RR.family_tolerance(cases, "outdoor_5deg")
    T, ok = robust_transform(p0, p1, device=DEV)
    T2, _ = robust_transform(p0, p1, device=DEV)
    dR, dt = _gaps(T, RR.robust_transform_f64(p0, p1))
    print(f"n={n}: vs fp64 restatement |dR| {dR:.2e} (tol {tol_R:.2e}) |dt| {dt:.2e} (tol {tol_t:.2e})")
    assert ok and T.tobytes() == T2.tobytes()
    assert dR <= tol_R and dt <= tol_t
    assert np.linalg.norm(T[:3, 3] - planted[:3, 3]) < 0.02
