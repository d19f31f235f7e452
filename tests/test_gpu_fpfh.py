"""imf_fpfh_features on the GPU against the NumPy restatement (tests/fpfh_restate.py), on the device's own neighbour lists
and normals (`estimate_normals`): the integer SPFH counts exactly, the descriptor to one fp32 rounding, on every point the
restatement can decide; the padded width, the run-to-run bytes, a corrupt list, the wrapper's refusals.  The time of one
call on the fixture case is printed, not gated."""
import time

import numpy as np
import pytest

import fpfh_restate as FR

pytestmark = pytest.mark.gpu

CASES = FR.cases()
IDS = [c.name for c in CASES]
_GPU = {}


def _inputs(case):
    """(normals, nbr, counts) of a case from the device, and the restatement on them: once per process, left unchanged."""
    from imfnet_amd.matching import estimate_normals
    if case.name not in _GPU:
        _, counts, nbr = estimate_normals(case.points, knn=case.knn, max_radius=case.radius, return_neighbors=True)
        nrm = case.normals
        if nrm is None:
            nrm, _ = estimate_normals(case.points, knn=30, max_radius=case.radius, viewpoint=FR.VIEWPOINT)
        _GPU[case.name] = (nrm, nbr, counts, FR.restate(case.points, nrm, nbr, counts))
    return _GPU[case.name]


def _entry(points, normals, nbr, counts, width, with_hist, repeat=1):
    """The C entry on given lists (no search).  Returns (out, hist or None, milliseconds per call by device events)."""
    import torch
    from imfnet_amd import _lib
    from imfnet_amd._lib import check
    dev = torch.device("cuda")
    p = torch.as_tensor(np.ascontiguousarray(points, np.float64), device=dev)
    q = torch.as_tensor(np.ascontiguousarray(normals, np.float64), device=dev)
    nb = torch.as_tensor(np.ascontiguousarray(nbr, np.int32), device=dev)
    ct = torch.as_tensor(np.ascontiguousarray(counts, np.int32), device=dev)
    n, knn = nb.shape
    L = _lib.lib()
    nbytes = L.imf_fpfh_workspace_bytes(n, knn)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.full((n, width), -1.0, dtype=torch.float32, device=dev)
    hist = torch.full((n, 33), -1, dtype=torch.int32, device=dev) if with_hist else None
    st = torch.cuda.current_stream().cuda_stream
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(repeat):
        check(L.imf_fpfh_features(p.data_ptr(), q.data_ptr(), n, nb.data_ptr(), ct.data_ptr(), knn, width, out.data_ptr(),
                                  hist.data_ptr() if with_hist else None, ws.data_ptr(), nbytes, st), "imf_fpfh_features")
    t1.record()
    torch.cuda.synchronize()
    return out.cpu().numpy(), hist.cpu().numpy() if with_hist else None, t0.elapsed_time(t1) / repeat


def _compare(out, hist, ref, name):
    clean = ref["clean"]
    if hist is not None:
        assert np.array_equal(hist.sum(1), 3 * ref["m"]), name
        assert np.array_equal(hist[clean], ref["hist"][clean]), name
    want = ref["out"][clean]
    err = np.abs(out[clean, :33].astype(np.float64) - want)
    tol = 2.0 ** -23 * np.abs(want) + 1e-12
    worst = float((err / tol).max(initial=0.0))
    print(f"\n{name}: n = {len(clean)}, non-clean share {1.0 - clean.mean():.4%}, worst error / tolerance {worst:.3f}")
    assert (err <= tol).all(), (name, worst)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fpfh_matches_the_restatement(case, capsys):
    from imfnet_amd.matching import compute_fpfh
    nrm, nbr, counts, ref = _inputs(case)
    kw = dict(normals=nrm, radius=case.radius, max_nn=case.knn)
    out64, hist = compute_fpfh(case.points, width=64, return_hist=True, **kw)
    out33 = compute_fpfh(case.points, width=33, **kw)
    assert out64.is_cuda and out64.dtype.is_floating_point and tuple(out64.shape) == (len(case.points), 64)
    assert tuple(out33.shape) == (len(case.points), 33) and tuple(hist.shape) == (len(case.points), 33)
    out64, out33, hist = out64.cpu().numpy(), out33.cpu().numpy(), hist.cpu().numpy()
    assert out64.dtype == np.float32 and hist.dtype == np.int32
    with capsys.disabled():
        _compare(out64, hist, ref, case.name)
    assert out64[:, 33:].tobytes() == bytes(4 * 31 * len(case.points))          # +0.0f, not -0.0f
    assert out33.tobytes() == np.ascontiguousarray(out64[:, :33]).tobytes()
    again, hist2 = compute_fpfh(case.points, width=64, return_hist=True, **kw)
    assert again.cpu().numpy().tobytes() == out64.tobytes() and hist2.cpu().numpy().tobytes() == hist.tobytes()
    assert 1.0 - ref["clean"].mean() <= 0.01                                   # the cap holds on the device's normals too
    assert np.isfinite(out64).all() and not out64[ref["m"] == 0].any()


def test_estimated_normals_path_equals_the_given_normals_path():
    from imfnet_amd.matching import compute_fpfh
    case = {c.name: c for c in CASES}["curved_patch_knn64"]
    nrm = _inputs(case)[0]
    a = compute_fpfh(case.points, normals=nrm, radius=case.radius, max_nn=case.knn)
    b = compute_fpfh(case.points, radius=case.radius, max_nn=case.knn, normal_knn=30, viewpoint=FR.VIEWPOINT)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_entry_without_hist_output_and_its_time_on_the_fixture(capsys):
    """The counts then live in the workspace: the same descriptor bytes.  The time per call is printed, not gated."""
    case = {c.name: c for c in CASES}["fixture_every_16th"]
    nrm, nbr, counts, ref = _inputs(case)
    with_hist, hist, _ = _entry(case.points, nrm, nbr, counts, 64, True)
    without, _, _ = _entry(case.points, nrm, nbr, counts, 64, False)
    assert with_hist.tobytes() == without.tobytes()
    with capsys.disabled():
        _compare(with_hist, hist, ref, case.name + " (entry)")
    _, _, ms = _entry(case.points, nrm, nbr, counts, 64, False, repeat=20)
    from imfnet_amd.matching import compute_fpfh
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    compute_fpfh(case.points, normals=nrm, radius=case.radius, max_nn=case.knn, width=64)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\nimf_fpfh_features, n = {len(case.points)}, knn = {case.knn}: {ms * 1e3:.1f} us per call (device events, "
              f"mean of 20); compute_fpfh with its neighbour search and host copies: {wall * 1e3:.2f} ms")


def test_corrupt_list_entries_are_skipped():
    """Entries outside [0, n) are read as padding: the kernels check the index before every use of it."""
    case = {c.name: c for c in CASES}["isolated_trio"]
    nrm, nbr, counts, _ = _inputs(case)
    n = len(case.points)
    bad = np.array(nbr, np.int32)
    g = np.random.default_rng(4)
    hit = g.random(bad.shape) < 0.1
    bad[hit] = g.choice(np.array([n, n + 5, -7, 2 ** 31 - 1, -2 ** 31], np.int64), int(hit.sum())).astype(np.int32)
    ref = FR.restate(case.points, nrm, bad, counts)
    assert (ref["m"] < FR.restate(case.points, nrm, nbr, counts)["m"]).any()
    out, hist, _ = _entry(case.points, nrm, bad, counts, 33, True)
    _compare(out, hist, ref, "corrupt list")


def test_wrapper_refuses_bad_arguments():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.matching import compute_fpfh
    pts = CASES[0].points
    with pytest.raises(ImfError):
        compute_fpfh(pts, max_nn=65)
    with pytest.raises(ImfError):
        compute_fpfh(pts, width=32)
    with pytest.raises(ImfError):
        compute_fpfh(pts, normals=np.zeros((3, 3)))
