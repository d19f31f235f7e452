"""Fragment overlap on the GPU (csrc/overlap.hip through imfnet_amd/overlap.py) against the NumPy restatement
(tests/overlap_restate.py): a sequence of slabs cut from the fixture fragment, a cell denser than one LDS tile, and
frames -> fragments -> pair lists -> IndoorPairDataset end to end.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overlap_restate as R   # noqa: E402
import tsdf_scene as S        # noqa: E402

pytestmark = pytest.mark.gpu

THRESH, MIN_OVERLAP, MAX_POINTS = 0.075, 0.3, 30000


@pytest.fixture(scope="module")
def sequence(clouds):
    frags, numbers = R.slab_sequence(clouds[0], MAX_POINTS)
    return frags, numbers


@pytest.fixture(scope="module")
def restated(sequence):
    frags, numbers = sequence
    counts = {}
    kept = R.sequence_overlap(frags, THRESH, MIN_OVERLAP, numbers, counts)
    return kept, counts


@pytest.fixture(scope="module")
def engine(sequence):
    from imfnet_amd.overlap import sequence_overlap
    frags, numbers = sequence
    stats = {}
    kept = sequence_overlap(frags, THRESH, MIN_OVERLAP, numbers=numbers, stats=stats)
    return kept, stats


def _ratio(n, frags, i, j):
    return n / max(len(frags[i]), len(frags[j]))


def test_the_sequence_holds_every_case(sequence, restated):
    """The conditions on the input, from the restatement alone: kept pairs, pairs the ratio rejects after the exact
    pass, pairs the bound alone rejects (one of them with correspondences), a consecutive pair with a high overlap that
    forms no pair, a fragment that was down-sampled, and no two fragments with all their points in common."""
    frags, numbers = sequence
    kept, counts = restated
    from imfnet_amd.overlap import CELL_MARGIN
    cell = float(np.float32(THRESH)) * CELL_MARGIN
    assert len(frags) == 8 and all(20000 <= len(f) <= MAX_POINTS for f in frags) and len(frags[7]) == MAX_POINTS
    assert set(counts) == set(R.candidate_pairs(numbers)) and len(counts) == 21
    bound = {k: R.cell_bound(frags[k[0]], frags[k[1]], cell) for k in counts}
    assert all(bound[k] >= counts[k] for k in counts)
    by_bound = [k for k in counts if _ratio(bound[k], frags, *k) < MIN_OVERLAP]
    by_ratio = [k for k in counts if k not in by_bound and k not in kept]
    print(f"kept {sorted(kept)}\nrejected by the ratio {by_ratio}\nrejected by the bound {by_bound}")
    assert len(kept) >= 2 and len(by_ratio) >= 2 and len(by_bound) >= 1
    assert any(counts[k] > 0 for k in by_bound)
    assert (0, 1) not in counts
    assert _ratio(len(R.correspondences_windowed(frags[0], frags[1], THRESH)), frags, 0, 1) > 0.9
    for i in range(8):
        for j in range(i + 1, 8):
            assert frags[i].shape != frags[j].shape or not np.array_equal(frags[i], frags[j])


def test_kept_pairs_equal_the_restatement(sequence, restated, engine):
    frags, _ = sequence
    want, counts = restated
    got, stats = engine
    assert set(got) == set(want)
    for k in sorted(want):
        ratio, rows = got[k]
        print(f"pair {k}: {len(rows)} rows, ratio {ratio!r} (restated {want[k][0]!r})")
        assert rows.dtype == np.int64 and rows.shape == want[k][1].shape
        assert np.array_equal(rows, want[k][1])
        assert isinstance(ratio, float) and ratio == want[k][0]
    # every exact pass that ran found the restatement's count, kept or not
    assert all(stats["exact"][k] == counts[k] for k in stats["exact"])


def test_bound_is_an_upper_bound_and_rejects_no_kept_pair(sequence, restated, engine):
    from imfnet_amd.overlap import CELL_MARGIN
    frags, numbers = sequence
    want, counts = restated
    _, stats = engine
    cell = float(np.float32(THRESH)) * CELL_MARGIN
    assert set(stats["bound"]) == set(counts)
    for k in sorted(counts):
        print(f"pair {k}: bound {stats['bound'][k]}, exact {counts[k]}")
        assert stats["bound"][k] >= counts[k]
        assert stats["bound"][k] == R.cell_bound(frags[k[0]], frags[k[1]], cell)
    assert set(stats["exact"]) >= set(want)
    assert len(stats["exact"]) < len(counts)                             # the bound did reject something


def test_two_runs_are_identical_and_the_prefilter_changes_nothing(sequence, engine):
    from imfnet_amd.overlap import sequence_overlap
    frags, numbers = sequence
    got, _ = engine
    stats = {}
    for kw in (dict(), dict(prefilter=False, stats=stats)):
        again = sequence_overlap(frags, THRESH, MIN_OVERLAP, numbers=numbers, **kw)
        assert set(again) == set(got)
        for k in got:
            assert again[k][0] == got[k][0] and again[k][1].tobytes() == got[k][1].tobytes()
    assert len(stats["exact"]) == 21


def test_a_cell_denser_than_one_lds_tile(clouds):
    """5000 points of p and 700 queries inside one 7.5 cm cell (several LDS tiles of 1024, several query chunks of 256),
    duplicates among them, next to ordinary surface points."""
    import torch
    from imfnet_amd.overlap import pair_overlap, build_indices
    rng = np.random.default_rng(4)
    base = clouds[0][::60].astype(np.float32)
    centre = np.float32(0.075) * np.floor(base[100] / np.float32(0.075)) + np.float32(0.0375)
    dense_p = (centre + (rng.random((5000, 3)) - 0.5) * 0.06).astype(np.float32)
    dense_p[2500:2600] = dense_p[100:200]                                # equal points: ties go to the lowest index
    dense_q = (centre + (rng.random((700, 3)) - 0.5) * 0.07).astype(np.float32)
    dense_q[:50] = dense_p[100:150]                                      # distance 0 to two points of p each
    p = np.concatenate([base, dense_p])
    q = np.concatenate([dense_q, clouds[0][7::90].astype(np.float32)])
    ip, iq = build_indices([p, q], THRESH)
    tab_off = ip.desc.table - ip.storage.data_ptr()
    counts = ip.storage[tab_off:tab_off + 16 * ip.desc.capacity].view(torch.int32)[3::4]     # imf_slot.pad
    assert int(counts.max()) >= 5000 and int(counts.sum()) == len(p) == ip.meta[3]
    assert iq.n_chunks >= iq.n_cells + 2
    n, rows = pair_overlap(ip, iq, THRESH)
    want = R.correspondences(p, q, THRESH)
    assert n == len(want) and np.array_equal(rows.cpu().numpy(), want)
    assert (want[:50, 0] == len(base) + 100 + np.arange(50)).all()


def test_edge_cases(clouds):
    import torch
    from imfnet_amd import _lib
    from imfnet_amd.overlap import FragmentIndex, pair_overlap, sequence_overlap
    a = clouds[0][::200].astype(np.float32)
    far = a + np.float32(50.0)
    assert sequence_overlap([a, a, far], THRESH, MIN_OVERLAP) == {}      # (0, 2) only: nothing near
    got = sequence_overlap([a, far, a], THRESH, MIN_OVERLAP)              # (0, 2): a fragment and itself
    assert list(got) == [(0, 2)] and got[(0, 2)][0] == 1.0
    assert np.array_equal(got[(0, 2)][1], R.correspondences(a, a, THRESH))
    assert sequence_overlap([a, np.zeros((0, 3), np.float32), a[:0], a], THRESH, MIN_OVERLAP).keys() == {(0, 3)}
    with pytest.raises(_lib.ImfError):
        bad = a.copy()
        bad[3, 1] = np.nan
        FragmentIndex(torch.from_numpy(bad), 0.0751).meta
    # a cell edge at or below the threshold is refused, nothing launched
    small = FragmentIndex(torch.from_numpy(a), 0.075)
    with pytest.raises(_lib.ImfError, match="cell"):
        pair_overlap(small, small, THRESH)
    torch.cuda.synchronize()


def test_frames_to_fragments_to_pairs_to_the_training_set(tmp_path):
    """DESIGN.md 12's chain made true: a raw RGB-D tree is fused into fragments, compute_overlap moves them into one
    frame and writes the pair list, and IndoorPairDataset reads it: every listed pair has positive pairs under the
    identity."""
    from imfnet_amd import compute_overlap as CO
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.train.data import IndoorPairDataset
    from imfnet_amd.train.trainer import parse_config
    raw, frag = str(tmp_path / "raw"), str(tmp_path / "frag")
    S.write_tree(raw, S.make_sequence(160, 120, n_frames=8, arc=0.5))
    cfg = FF.parse_args(["--dataset_root", raw, "--out_root", frag, "--height", "120", "--width", "160", "--frames_per_frag",
                         "2", "--voxel_length", "0.006", "--lattice_offset", "0", "--write_image"])
    assert FF.run(cfg, log=lambda s: None) == 4
    world, out, lists = str(tmp_path / "world"), str(tmp_path / "out"), str(tmp_path / "lists")
    cfg = CO.parse_args(["--dataset_root", frag, "--out_root", out, "--list_root", lists, "--world_root", world,
                         "--max_points", "40000"])
    written = CO.run(cfg, log=lambda s: None)
    assert written == 3                                                  # (0, 2), (0, 3), (1, 3): the poses see one room
    config = parse_config(["--threed_match_dir", world, "--overlap_path", lists])
    ds = IndoorPairDataset("val", ["scene-a"], config, seed=0, device="cuda:0")
    assert len(ds) == written
    for n in range(len(ds)):
        f0, f1 = ds.files[n]
        rows = np.load(os.path.join(out, "scene-a", "seq-01", f"{os.path.basename(f0)[:-4]}-{os.path.basename(f1)[:-4]}.npy"))
        item = ds[n]
        print(f"{f0} {f1}: {len(rows)} correspondences, {item['matches'].shape[0]} positive pairs")
        assert len(rows) > 0 and item["matches"].shape[0] > 0
        assert np.array_equal(item["trans"], np.identity(4))
    # a plain run over world_root: byte-identical outputs on the device path too
    cfg = CO.parse_args(["--dataset_root", world, "--out_root", str(tmp_path / "out2"), "--list_root", str(tmp_path / "lists2"),
                         "--max_points", "40000"])
    assert CO.run(cfg, log=lambda s: None) == written
    for name in os.listdir(os.path.join(out, "scene-a", "seq-01")):
        with open(os.path.join(out, "scene-a", "seq-01", name), "rb") as f0, \
                open(tmp_path / "out2" / "scene-a" / "seq-01" / name, "rb") as f1:
            assert f0.read() == f1.read()
    assert (tmp_path / "lists2" / "scene-a@seq-01-0.30.txt").read_bytes() == \
        open(os.path.join(lists, "scene-a@seq-01-0.30.txt"), "rb").read()
