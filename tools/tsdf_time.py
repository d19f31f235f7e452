"""Time of the fragment fusion (imfnet_amd/fuse.py, csrc/tsdf.hip) on one synthetic fragment of 50 frames at 640 x 480
(tests/tsdf_scene.py), next to the NumPy restatement (tests/tsdf_restate.py) on the same input.

  allocate / integrate / extract   each call between device synchronisations, inputs resident (medians)
  mesh                              TSDFVolume.extract_mesh on the same volume: the count call, the sized call, the download
  mesh_device                       the sized imf_tsdf_mesh call alone, buffers resident (cells, count, two scans, two writes)
  fragment                          fuse_fragment host to host: upload of the depth frames, the three calls, the download
  restatement                       the NumPy restatement, its units split over at most 16 threads (one run)
  integrate_bytes_per_s             units x 4096 voxels x 8 B read and written once, over the integrate time
  --color                           the same legs again on a coloured volume of the same input, in the same process
                                    (tests/tsdf_color_scene.py paints the frames): color_allocate / integrate / extract /
                                    mesh / fragment _ms, and each as a ratio to the depth-only leg of this run

Usage: python tools/tsdf_time.py [--iters 5] [--warmup 2] [--frames 50] [--no-restatement] [--color] [--out FILE.json]
Prints one JSON line (milliseconds, medians)."""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def mesh_device_call(vol, n_vertices, n_triangles):
    """One sized imf_tsdf_mesh call on resident buffers, as a function to time."""
    import ctypes as C
    L, dev = vol.L, vol.device
    p = lambda t: C.c_void_p(t.data_ptr())
    ws = torch.empty(L.imf_tsdf_mesh_workspace_bytes(vol.n_units), dtype=torch.uint8, device=dev)
    out_n = torch.zeros(2, dtype=torch.int64, device=dev)
    v = torch.empty((max(1, n_vertices), 3), dtype=torch.float64, device=dev)
    t = torch.empty((max(1, n_triangles), 3), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        rc = L.imf_tsdf_mesh(p(vol._voxels), p(vol._units), p(vol._meta), vol.n_units, p(vol._table), vol.table_capacity,
                             C.byref(vol.params), p(v), len(v), p(t), len(t), p(out_n), p(ws), ws.numel(), stream)
        assert rc == 0
    return call


def restate_threaded(R, seq, threads):
    p = R.params()
    c2w = seq["poses"]
    units = R.allocate(seq["depth"], c2w, seq["K"], p)
    w2c = np.linalg.inv(c2w)
    chunks = np.array_split(np.arange(len(units)), max(1, min(len(units) // 64, threads * 4)))
    with cf.ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda ix: R.integrate(units[ix], seq["depth"], w2c, seq["K"], p), chunks))
    tsdf, w = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    return R.extract(units, tsdf, w, p)[0], units


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--color", action="store_true", help="also time a coloured volume on the same input")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import tsdf_restate as R
    import tsdf_scene as S
    from imfnet_amd.fuse import TSDFVolume, fuse_fragment
    assert torch.cuda.is_available(), "tsdf_time needs a GPU"
    seq = S.make_sequence(640, 480, n_frames=a.frames, arc=1.2)
    H, W = seq["depth"].shape[1:]
    res = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "height": H, "width": W, "iters": a.iters,
           "warmup": a.warmup, "voxel_length": 3.0 / 512, "lattice_offset": 0.5}
    dev = torch.device("cuda:0")
    d = torch.from_numpy(seq["depth"].view(np.int16)).to(dev)
    state = {}

    def allocate():
        state["vol"] = TSDFVolume(seq["K"], H, W, unit_capacity=1 << 16)
        state["vol"].allocate(d, seq["poses"])

    def integrate():
        state["vol"]._voxels = None                           # a fresh volume each time: the same work every iteration
        state["vol"].integrate(d, seq["poses"])

    res["allocate_ms"] = median_ms(allocate, a.iters, a.warmup)
    res["integrate_ms"] = median_ms(integrate, a.iters, a.warmup)
    res["extract_ms"] = median_ms(lambda: state["vol"].extract(), a.iters, a.warmup)
    pts = state["vol"].extract()
    res["units"], res["points"] = state["vol"].n_units, int(len(pts))
    res["mesh_ms"] = median_ms(lambda: state["vol"].extract_mesh(), a.iters, a.warmup)
    verts, tris = state["vol"].extract_mesh()
    res["mesh_vertices"], res["mesh_triangles"] = int(len(verts)), int(len(tris))
    res["mesh_device_ms"] = median_ms(mesh_device_call(state["vol"], len(verts), len(tris)), a.iters, a.warmup)
    res["mesh_over_extract"] = res["mesh_ms"] / res["extract_ms"]
    res["integrate_state_bytes"] = res["units"] * 4096 * 8 * 2
    res["integrate_bytes_per_s"] = res["integrate_state_bytes"] / (res["integrate_ms"] * 1e-3)
    res["voxel_frame_updates_per_s"] = res["units"] * 4096 * a.frames / (res["integrate_ms"] * 1e-3)
    res["fragment_ms"] = median_ms(lambda: fuse_fragment(seq["depth"], seq["poses"], seq["K"]), a.iters, a.warmup)
    if a.color:
        import tsdf_color_scene as CS
        rgb = CS.make_colors(seq)
        c = torch.from_numpy(rgb).to(dev)

        def color_allocate():
            state["cvol"] = TSDFVolume(seq["K"], H, W, unit_capacity=1 << 16, color=True)
            state["cvol"].allocate(d, seq["poses"])

        def color_integrate():
            state["cvol"]._voxels = state["cvol"]._colors = None
            state["cvol"].integrate(d, seq["poses"], c)

        res["color_allocate_ms"] = median_ms(color_allocate, a.iters, a.warmup)
        res["color_integrate_ms"] = median_ms(color_integrate, a.iters, a.warmup)
        res["color_extract_ms"] = median_ms(lambda: state["cvol"].extract(colors=True), a.iters, a.warmup)
        res["color_mesh_ms"] = median_ms(lambda: state["cvol"].extract_mesh(colors=True), a.iters, a.warmup)
        res["color_fragment_ms"] = median_ms(lambda: fuse_fragment(seq["depth"], seq["poses"], seq["K"], color=rgb), a.iters,
                                             a.warmup)
        res["color_points_equal"] = bool(np.array_equal(state["cvol"].extract(colors=True)[0], pts))
        res["color_state_bytes"] = res["units"] * 4096 * 20 * 2
        for leg in ("allocate", "integrate", "extract", "mesh", "fragment"):
            res[f"color_{leg}_ratio"] = res[f"color_{leg}_ms"] / res[f"{leg}_ms"]
    if not a.no_restatement:
        threads = min(16, len(os.sched_getaffinity(0)))
        t = time.perf_counter()
        ref, units = restate_threaded(R, seq, threads)
        res["restatement_ms"], res["restatement_threads"] = (time.perf_counter() - t) * 1e3, threads
        res["restatement_units_equal"] = bool(units.shape == state["vol"].units.shape and (units == state["vol"].units).all())
        res["restatement_points"] = int(len(ref))
        if ref.shape == pts.shape:
            res["max_abs_diff_vs_restatement"] = float(np.abs(ref - pts).max())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
