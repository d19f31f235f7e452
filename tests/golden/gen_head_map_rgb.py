"""Writes head_map_rgb.npz and head_map_ply.json from the reference's files/3D_head_map.ply (run by hand:
`python tests/golden/gen_head_map_rgb.py <reference checkout>`): the colours DAM wrote for fragment 0, target row 780,
row for row with head_map_xyz.npz, and the SHA-256 / byte length of the file itself.  No test reads the reference."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    path = os.path.join(ref, "files", "3D_head_map.ply")
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").split("\n")
    assert header[1] == "format binary_little_endian 1.0"
    n = int([l for l in header if l.startswith("element vertex")][0].split()[-1])
    props = [l.split()[1:] for l in header if l.startswith("property")]
    assert props == [["double", "x"], ["double", "y"], ["double", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    rows = np.frombuffer(raw[end:], dtype=np.dtype([("xyz", "<f8", 3), ("rgb", "u1", 3)]))
    assert len(rows) == n
    xyz = np.load(os.path.join(HERE, "head_map_xyz.npz"))["xyz"]
    assert (rows["xyz"] == xyz.astype(np.float64)).all(), "rows do not correspond to head_map_xyz.npz"
    np.savez_compressed(os.path.join(HERE, "head_map_rgb.npz"), rgb=np.ascontiguousarray(rows["rgb"]))
    with open(os.path.join(HERE, "head_map_ply.json"), "w") as f:
        json.dump({"file": "files/3D_head_map.ply", "bytes": len(raw), "sha256": hashlib.sha256(raw).hexdigest(),
                   "vertices": n, "target_row": 780}, f, indent=1)
        f.write("\n")
    print(f"{n} rows, {len(raw)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
