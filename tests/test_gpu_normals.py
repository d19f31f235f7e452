"""imf_estimate_normals (csrc/normals.hip) against the NumPy restatement (tests/normals_restate.py) on its catalogue:
the neighbour lists and counts exactly, the normals by the gates of normals_restate.check_normals (unit length, Rayleigh
quotient against numpy.linalg.eigh, 1e-9 rad to the restatement where the eigenvalue gap decides the direction, the sign
rules), bit-identical repeats, the error flag."""
import numpy as np
import pytest

import normals_restate as NR

pytestmark = pytest.mark.gpu

CASES = NR.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lists_are_exact_and_normals_pass_the_gates(case):
    from imfnet_amd.matching import estimate_normals
    ref = NR.reference(case, None)
    nrm, counts, nbr = estimate_normals(case.points, case.knn, case.max_radius, return_neighbors=True)
    assert nbr.shape == (len(case.points), case.knn) and nbr.dtype == np.int32 and counts.dtype == np.int32
    assert np.array_equal(counts, ref["counts"])
    assert np.array_equal(nbr, ref["nbr"])
    got = NR.check_normals(nrm, case.points, ref, None)
    print(f"{case.name}: n={len(case.points)} knn={case.knn} {got}")
    if case.generic:
        assert got["under_gap"] <= 0.10
    # facing a viewpoint: the same lists, the other sign rule
    nrm_v, counts_v = estimate_normals(case.points, case.knn, case.max_radius, viewpoint=NR.VIEWPOINT)
    assert np.array_equal(counts_v, counts)
    NR.check_normals(nrm_v, case.points, NR.reference(case, NR.VIEWPOINT), NR.VIEWPOINT)
    same = np.abs((nrm * nrm_v).sum(1))
    assert (np.abs(nrm_v) == np.abs(nrm)).all() and (same > 0.5).all()     # only the sign differs
    # a second call gives the same bits
    again = estimate_normals(case.points, case.knn, case.max_radius, return_neighbors=True)
    assert again[0].tobytes() == nrm.tobytes() and again[1].tobytes() == counts.tobytes() and again[2].tobytes() == nbr.tobytes()


def test_a_point_beyond_the_grid_or_nan_raises():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.matching import estimate_normals
    pts = np.random.default_rng(0).uniform(0, 1, (50, 3))
    edge = 0.25 / 2
    for bad in (np.nan, (1 << 17) * edge, -(1 << 17) * edge - edge):
        p = pts.copy()
        p[17, 1] = bad
        with pytest.raises(ImfError):
            estimate_normals(p, 8, 0.25)
    p = pts.copy()
    p[17, 1] = ((1 << 17) - 1.5) * edge                                   # the last permitted cell
    nrm, counts = estimate_normals(p, 8, 0.25)
    assert counts[17] == 1 and (nrm[17] == [0.0, 0.0, 1.0]).all()
    with pytest.raises(ImfError):
        estimate_normals(pts, 65, 0.25)
    with pytest.raises(ImfError):
        estimate_normals(pts, 8, float("inf"))
