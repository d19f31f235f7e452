"""The training-pair builder, the parts that need no GPU: the exported entry points, the NumPy restatement
(tests/overlap_restate.py) on a hand-made case, the seeded down-sampling, and the command line's tree walk
(imfnet_amd/compute_overlap.py) driven by the restatement instead of the device."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import overlap_restate as R   # noqa: E402

T32 = np.float32(0.075)


def test_header_declares_the_overlap_entry_points():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    for name in ("imf_overlap_index_bytes", "imf_overlap_index_workspace_bytes", "imf_overlap_index_build",
                 "imf_overlap_bound", "imf_overlap_pair", "imf_overlap_emit_workspace_bytes", "imf_overlap_emit"):
        assert re.search(r"\b%s\(" % name, text) and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    body = text[text.index("typedef struct imf_overlap_index {"):text.index("} imf_overlap_index;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for n in re.findall(r"(?:imf_slot|int64_t|float|int32_t|double)\s+([^;]+);", body)]
    assert names == [f[0] for f in _lib.OverlapIndex._fields_]
    L = _lib.lib()
    assert L.imf_overlap_index_bytes(0) == 0 and L.imf_overlap_index_bytes(-5) == 0
    assert L.imf_overlap_index_workspace_bytes(0) == 0 and L.imf_overlap_emit_workspace_bytes(0) == 0
    # table (16 B x capacity) + xyz + idx + cells + chunks + meta, each rounded up to 256 bytes
    n = 300000
    cap = L.imf_hash_capacity(n)
    r = lambda v: (v + 255) // 256 * 256
    assert L.imf_overlap_index_bytes(n) == r(16 * cap) + r(12 * n) + r(4 * n) + r(4 * n) + r(8 * n) + 256
    assert L.imf_overlap_emit_workspace_bytes(n) == r(4 * ((n + 1023) // 1024))


def test_restatement_on_a_hand_made_case():
    """p (index: point)                      q (index: point)
       0: (0.1, 0, 0)                        0: (0.05, 0, 0)    0.1f - 0.05f == 0.05f exactly: p0, p1, p5 tie -> p0
       1: (0, 0, 0)                          1: (0, 5, 0)       p2 at exactly float32(0.075): kept
       2: (t, 5, 0)        t = float32(.075) 2: (0, 9, 0)       p3 one float32 step farther: dropped
       3: (next(t), 9, 0)                    3: (0.02, 0, 0)    p1 and p5 tie at 0.02 -> p1
       4: (3, 3, 3)                          4: (3.01, 3.02, 3.03)  p4
       5: (0, 0, 0)                          5: (-7, 0, 0)      nothing near: dropped
                                             6: (3, 3, 3.1)     p4 at 0.1: dropped"""
    t = T32
    t_next = np.nextafter(t, np.float32(1))
    p = np.array([[0.1, 0, 0], [0, 0, 0], [t, 5, 0], [t_next, 9, 0], [3, 3, 3], [0, 0, 0]], np.float32)
    q = np.array([[0.05, 0, 0], [0, 5, 0], [0, 9, 0], [0.02, 0, 0], [3.01, 3.02, 3.03], [-7, 0, 0], [3, 3, 3.1]], np.float32)
    assert np.float32(0.1) - np.float32(0.05) == np.float32(0.05)
    assert np.sqrt(t * t) == t and np.sqrt(t_next * t_next) == t_next > t
    idx, d2 = R.nearest(p, q)
    assert idx.tolist() == [0, 2, 3, 1, 4, 1, 4]
    assert d2[1] == t * t and d2[2] == t_next * t_next and d2.dtype == np.float32
    want = np.array([[0, 0], [2, 1], [1, 3], [4, 4]], np.int64)
    for rows in (R.correspondences(p, q, 0.075), R.correspondences_windowed(p, q, 0.075)):
        assert rows.dtype == np.int64 and np.array_equal(rows, want)
    assert R.overlap_ratio(4, len(p), len(q)) == 4 / 7
    # the prefilter restated: q5 and q6 (two cells above p4 in z) have no cell of p around theirs, the others have
    assert R.cell_bound(p, q, 0.0751) == 5
    # the pair loop: consecutive numbers are left out, whatever their position in the list
    assert R.candidate_pairs([0, 1, 2, 5, 6, 10]) == [(0, 2), (0, 3), (0, 4), (0, 5), (1, 3), (1, 4), (1, 5), (2, 3),
                                                       (2, 4), (2, 5), (3, 5), (4, 5)]


def test_windowed_restatement_equals_the_brute_force(clouds):
    a, b = clouds[0][5::40], clouds[0][::40]
    rows = R.correspondences(a, b, 0.075)
    assert 1000 < len(rows) < len(b) and np.array_equal(rows, R.correspondences_windowed(a, b, 0.075))
    assert len(rows) <= R.cell_bound(a, b, 0.0751)


def test_downsample_is_seeded_and_order_independent():
    from imfnet_amd.overlap import downsample, seed_of
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((1000, 3))
    for cap in (1000, 5000):
        out, ind = downsample(pts, cap, (0, "s", "q", "cloud_bin_0"))
        assert out.dtype == np.float32 and ind.dtype == np.int64
        assert np.array_equal(ind, np.arange(1000)) and np.array_equal(out, pts.astype(np.float32))
    key = (7, "scene-a", "seq-01", "cloud_bin_3")
    out, ind = downsample(pts, 300, key)
    assert out.shape == (300, 3) and out.dtype == np.float32 and len(np.unique(ind)) == 300
    assert np.array_equal(out, pts[ind].astype(np.float32))
    downsample(pts, 300, (7, "scene-a", "seq-01", "cloud_bin_2"))        # other draws in between change nothing
    again = downsample(pts, 300, key)
    assert np.array_equal(again[1], ind) and np.array_equal(again[0], out)
    other = downsample(pts, 300, (8,) + key[1:])
    assert not np.array_equal(other[1], ind)
    assert seed_of(key) == seed_of(list(key)) != seed_of((7, "scene-a", "seq-01", "cloud_bin_30"))
    assert R.downsample is downsample


def _write_fragments(root, numbers, rng, scene="scene-a", seq="seq-01"):
    """Fragments cut from one world cloud as slabs in x, each stored in a frame of its own next to its pose."""
    from scipy.spatial.transform import Rotation
    from imfnet_amd.fuse_fragments import write_ply
    world = rng.random((6000, 3)) * [2.0, 0.6, 0.3]
    folder = os.path.join(root, scene, seq)
    os.makedirs(folder, exist_ok=True)
    for n, k in enumerate(numbers):
        lo = 0.25 * n
        pts = world[(world[:, 0] >= lo) & (world[:, 0] < lo + 0.8)]
        pts = pts[rng.random(len(pts)) < (0.5, 0.25)[n % 2]]               # about 1200 and 600 points
        pose = np.eye(4)
        pose[:3, :3] = Rotation.from_rotvec(rng.standard_normal(3)).as_matrix()
        pose[:3, 3] = rng.standard_normal(3)
        local = (pts - pose[:3, 3]) @ pose[:3, :3]                       # pose . local = world
        write_ply(os.path.join(folder, f"cloud_bin_{k}.ply"), local)
        np.save(os.path.join(folder, f"cloud_bin_{k}.pose.npy"), pose)
        with open(os.path.join(folder, f"cloud_bin_{k}_0.jpg"), "wb") as f:
            f.write(b"image %d" % k)
    return folder


def _restated(cfg, clouds, numbers):
    return R.sequence_overlap(clouds, cfg.dist_thresh, cfg.min_overlap, numbers)


def _tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_tree_walk_with_the_restatement(tmp_path):
    from imfnet_amd import compute_overlap as CO
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.train.data import read_pair_files
    rng = np.random.default_rng(3)
    numbers = [0, 1, 2, 3, 10]                                           # alphanumeric: 10 after 3; 3 and 10 are no neighbours
    frag = str(tmp_path / "frag")
    _write_fragments(frag, numbers, rng)
    _write_fragments(frag, [0, 1, 2], rng, seq="seq-02")
    os.makedirs(tmp_path / "outA" / "scene-a" / "seq-02")                 # exists: skipped
    logs = []
    argsA = ["--dataset_root", frag, "--out_root", str(tmp_path / "outA"), "--list_root", str(tmp_path / "listA"),
             "--world_root", str(tmp_path / "world"), "--temp_root", str(tmp_path / "temp"), "--max_points", "700",
             "--threads", "2"]
    cfg = CO.parse_args(argsA)
    assert (cfg.dist_thresh, cfg.min_overlap, cfg.max_points, cfg.seed) == (0.075, 0.3, 700, 0)
    written = CO.run(cfg, overlap=_restated, log=logs.append)
    assert any("seq-02: Skip..." in s for s in logs)
    assert os.listdir(tmp_path / "outA" / "scene-a" / "seq-02") == [] and not (tmp_path / "world" / "scene-a" / "seq-02").exists()
    out = tmp_path / "outA" / "scene-a" / "seq-01"
    stems = [f"cloud_bin_{k}" for k in numbers]
    world = [read_ply_points(str(tmp_path / "world" / "scene-a" / "seq-01" / (s + ".ply"))).astype(np.float32) for s in stems]
    assert any(len(w) > 700 for w in world) and any(len(w) <= 700 for w in world)
    down = [CO.downsample(w, 700, (0, "scene-a", "seq-01", s)) for w, s in zip(world, stems)]
    for s, (pts, ind) in zip(stems, down):
        z = np.load(tmp_path / "temp" / "scene-a" / "seq-01" / (s + ".npz"))
        assert sorted(z.files) == ["indices", "points"]
        assert np.array_equal(z["points"], pts) and np.array_equal(z["indices"], ind) and z["points"].dtype == np.float32
    want = R.sequence_overlap([d[0] for d in down], 0.075, 0.3, numbers, pair_fn=R.correspondences)
    assert written == len(want) >= 2
    assert all(numbers[i] + 1 != numbers[j] for i, j in want) and (3, 4) in want          # cloud_bin_3 - cloud_bin_10
    # a consecutive pair overlaps well and is left out all the same
    assert len(R.correspondences(down[0][0], down[1][0], 0.075)) / max(len(down[0][0]), len(down[1][0])) >= 0.3
    names = set(os.listdir(out))
    assert names == {f"{stems[i]}-{stems[j]}{e}" for i, j in want for e in (".npy", "-overlap.txt")}
    for (i, j), (ratio, rows) in want.items():
        got = np.load(out / f"{stems[i]}-{stems[j]}.npy")
        assert got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 2 and np.array_equal(got, rows)
        assert (np.diff(got[:, 1]) > 0).all() and got[:, 0].max() < len(down[i][0]) and got[:, 1].max() < len(down[j][0])
        text = (out / f"{stems[i]}-{stems[j]}-overlap.txt").read_text()
        assert text == str(ratio) and float(text) == ratio == len(rows) / max(len(down[i][0]), len(down[j][0]))
    # the list: one file per sequence, read by the trainer into exactly the kept pairs, paths relative to world_root
    assert os.listdir(tmp_path / "listA") == ["scene-a@seq-01-0.30.txt"]
    pairs = read_pair_files(str(tmp_path / "listA"), ["scene-a"])
    assert pairs == [(f"scene-a/seq-01/{stems[i]}.ply", f"scene-a/seq-01/{stems[j]}.ply") for i, j in sorted(want)]
    lines = (tmp_path / "listA" / "scene-a@seq-01-0.30.txt").read_text().splitlines()
    assert [float(l.split()[2]) for l in lines] == [want[k][0] for k in sorted(want)]
    for a, b in pairs:
        assert os.path.exists(tmp_path / "world" / a) and os.path.exists(tmp_path / "world" / b)
    assert (tmp_path / "world" / "scene-a" / "seq-01" / "cloud_bin_10_0.jpg").read_bytes() == b"image 10"
    # the moved fragments agree where they overlap: that is what makes the identity a ground truth
    assert np.sqrt(R.nearest(world[0], world[1])[1]).min() < 1e-5
    # a plain run over world_root: byte-identical outputs
    cfgB = CO.parse_args(["--dataset_root", str(tmp_path / "world"), "--out_root", str(tmp_path / "outB"), "--list_root",
                          str(tmp_path / "listB"), "--max_points", "700", "--threads", "1"])
    assert CO.run(cfgB, overlap=_restated, log=logs.append) == written
    a, b = _tree_bytes(tmp_path / "outA"), _tree_bytes(tmp_path / "outB")
    assert a == b and len(a) == 2 * written
    assert _tree_bytes(tmp_path / "listA") == _tree_bytes(tmp_path / "listB")
    # another seed draws other points
    cfgC = CO.parse_args(["--dataset_root", str(tmp_path / "world"), "--out_root", str(tmp_path / "outC"), "--list_root",
                          str(tmp_path / "listC"), "--max_points", "700", "--seed", "1"])
    CO.run(cfgC, overlap=_restated, log=logs.append)
    assert _tree_bytes(tmp_path / "outC") != a


def test_threads_are_capped_by_the_quota_not_the_machine(tmp_path, monkeypatch):
    from imfnet_amd import compute_overlap as CO
    seen = []
    real = CO.cf.ThreadPoolExecutor
    monkeypatch.setattr(CO, "cpu_quota", lambda: 3)
    monkeypatch.setattr(CO.cf, "ThreadPoolExecutor", lambda n: (seen.append(n), real(n))[1])
    os.makedirs(tmp_path / "frag")
    cfg = CO.parse_args(["--dataset_root", str(tmp_path / "frag"), "--out_root", str(tmp_path / "o"), "--list_root",
                         str(tmp_path / "l"), "--threads", "64"])
    assert CO.run(cfg, overlap=_restated, log=lambda s: None) == 0
    assert seen == [3, 1]
