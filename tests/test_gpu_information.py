"""imf_information_matrix on the GPU against the NumPy restatement (tests/information_restate.py): bit for bit on integer
lattices, within the summation bound on general coordinates, the correspondence decisions of ICP one by one, the count
against ICP's own, the run-to-run bytes and the workspace refusal."""
import numpy as np
import pytest

import information_restate as IR

pytestmark = pytest.mark.gpu

CASES = IR.cases()
IDS = [c.name for c in CASES]
DECISIONS = IR.decision_cases()
_REF = {}


def _ref(case):
    """The restatement of a case: once per process, left unchanged."""
    if case.name not in _REF:
        _REF[case.name] = IR.restate(case.src, case.dst, case.T, case.r)
    return _REF[case.name]


def _entry(case, short=0):
    """The C entry.  Returns (status, info 6x6, meta [2], the 36 + 2 output values' bytes)."""
    import ctypes as C
    import torch
    from imfnet_amd import _lib
    dev = torch.device("cuda")
    s = torch.as_tensor(np.ascontiguousarray(case.src, np.float64), device=dev)
    d = torch.as_tensor(np.ascontiguousarray(case.dst, np.float64), device=dev)
    L = _lib.lib()
    nbytes = L.imf_information_workspace_bytes(len(s), len(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    info = torch.full((36,), -7.0, dtype=torch.float64, device=dev)
    meta = torch.full((2,), -7, dtype=torch.int32, device=dev)
    T = None if case.T is None else np.ascontiguousarray(case.T, np.float64)
    rc = L.imf_information_matrix(s.data_ptr(), len(s), d.data_ptr(), len(d), T.ctypes.data_as(C.c_void_p) if T is not None
                                  else None, float(case.r), info.data_ptr(), meta.data_ptr(), ws.data_ptr(), nbytes - short,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    info, meta = info.cpu().numpy(), meta.cpu().numpy()
    return rc, info.reshape(6, 6), meta, info.tobytes() + meta.tobytes()


def _check_structure(info, K):
    assert np.array_equal(info, info.T)
    assert np.array_equal(info[3:, 3:], K * np.eye(3))
    assert info[0, 3] == 0 and info[1, 4] == 0 and info[2, 5] == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matrix_against_the_restatement(case):
    """Integer lattices: every addend and every partial sum is an integer below 2^53, so the matrix is the restatement's
    bit for bit whatever the order.  General coordinates: the addends are the restatement's bit for bit (no contraction),
    so only the order of the K additions differs from math.fsum: |got - exact| <= K 2^-53 sum |addends| per entry."""
    from imfnet_amd.matching import icp_point_to_point, information_matrix
    ref = _ref(case)
    rc, info, meta, raw = _entry(case)
    assert rc == 0 and meta[1] == ref["flag"] == 0
    K = int(meta[0])
    assert K == ref["n_corr"], (K, ref["n_corr"])
    _check_structure(info, K)
    if case.exact:
        assert info.tobytes() == ref["info"].tobytes(), case.name
    else:
        err, tol = np.abs(info - ref["info"]), K * 2.0 ** -53 * ref["abs_sum"]
        print(f"\n{case.name}: K = {K}, worst error / bound {float((err[tol > 0] / tol[tol > 0]).max()):.4f}")
        assert (err <= tol).all(), (case.name, err, tol)
    if K == 0:
        assert info.tobytes() == np.zeros((6, 6)).tobytes()          # +0.0 everywhere
    # the wrapper, the run-to-run bytes, ICP's count of the same correspondences
    got, n_corr = information_matrix(case.src, case.dst, T=case.T, max_corr_dist=case.r)
    assert n_corr == K and got.tobytes() == info.tobytes()
    assert _entry(case)[3] == raw
    assert icp_point_to_point(case.src, case.dst, case.r, init=case.T, max_iteration=0)[4] == K


def test_decisions_of_the_correspondence_rule():
    from imfnet_amd.matching import icp_point_to_point, information_matrix

    def run(name):
        case = DECISIONS[name]
        ref = IR.restate(case.src, case.dst, case.T, case.r)
        rc, info, meta, _ = _entry(case)
        assert rc == 0 and meta[1] == 0 and meta[0] == ref["n_corr"], name
        assert info.tobytes() == ref["info"].tobytes(), name
        _check_structure(info, int(meta[0]))
        src = case.src[np.isfinite(case.src).all(1)]                # ICP's own count (a NaN row has no correspondence there
        assert icp_point_to_point(src, case.dst, case.r, init=case.T, max_iteration=0)[4] == meta[0], name   # either)
        return info, int(meta[0]), ref

    # d^2 = r^2 exactly (3-4-5): excluded; included at the next r up
    info, K, _ = run("at_r_excluded")
    assert K == 0 and info.tobytes() == np.zeros((6, 6)).tobytes()
    info, K, _ = run("at_r_next_up")
    assert K == 1 and np.array_equal(info, IR.information_from_points(DECISIONS["at_r_next_up"].dst[:1]))
    # two targets at the same distance: the lower index's point enters G, wherever it lies
    a, K, ref = run("tie_lowest_index")
    assert K == 1 and ref["j"][0] == 0 and np.array_equal(a, IR.information_from_points([[12.0, 20.0, 30.0]]))
    b, K, ref = run("tie_lowest_index_swapped")
    assert K == 1 and ref["j"][0] == 0 and np.array_equal(b, IR.information_from_points([[8.0, 20.0, 30.0]]))
    assert not np.array_equal(a, b)
    # duplicates of a target are one point for the matrix; NaN source rows are skipped
    _, K, _ = run("duplicate_targets")
    assert K == len(DECISIONS["duplicate_targets"].src)
    _, K, _ = run("nan_source_rows")
    assert K == len(DECISIONS["nan_source_rows"].src) - 2


def test_nan_target_raises_and_short_workspace_is_refused():
    from imfnet_amd import _lib
    from imfnet_amd._lib import ImfError
    from imfnet_amd.matching import information_matrix
    case = IR.nan_target_case()
    rc, _, meta, _ = _entry(case)
    assert rc == 0 and meta[1] == 1
    with pytest.raises(ImfError, match="NaN"):
        information_matrix(case.src, case.dst, max_corr_dist=case.r)
    rc, info, meta, _ = _entry(CASES[1], short=1)
    assert rc == -1 and b"workspace" in _lib.lib().imf_last_error()
    assert (info == -7.0).all() and (meta == -7).all()                # nothing was launched
    with pytest.raises(ImfError):
        information_matrix(np.zeros((0, 3)), case.dst)
