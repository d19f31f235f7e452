#!/usr/bin/env python3
"""Times of the RGB-D odometry quoted in DESIGN.md section 22:

    python tools/odometry_time.py [--reps 20] [--frames 50] [--track_reps 5]

The synthetic room of tests/tsdf_scene.py with the colours of tests/tsdf_color_scene.py at 640 x 480.  `pair`: one
rgbd_odometry_device call on two prepared frames (three levels, the default 20 / 10 / 5 iterations: 36 stages), `prepare`:
one prepare_frame from device images, each the median of --reps calls after a warm-up, device events around the call.
`track`: one `track` over --frames frames on an arc of 0.02 rad per frame, host images in, poses out (every frame uploaded
and prepared once, one device-to-host copy per pair), events and the host clock around the whole call, --track_reps calls
after one three-frame warm-up call (median, least and most); the poses' worst error against the ground truth goes with
it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--track_reps", type=int, default=5)
    a = ap.parse_args()
    import tsdf_color_scene as CS
    import tsdf_scene as S
    from imfnet_amd.odometry import prepare_frame, rgbd_odometry, rgbd_odometry_device, track
    seq = S.make_sequence(640, 480, n_frames=a.frames, seed=0, holes=0.02, arc=0.02 * (a.frames - 1))
    color = CS.make_colors(seq)
    d = [torch.from_numpy(seq["depth"][f].view(np.int16)).to("cuda") for f in (0, 1)]
    c = [torch.from_numpy(color[f]).to("cuda") for f in (0, 1)]
    res = dict(height=480, width=640, frames=a.frames)
    res["prepare"] = event_ms(lambda: prepare_frame(d[0], c[0], seq["K"]), a.reps)
    dst, src = (prepare_frame(d[f], c[f], seq["K"]) for f in (0, 1))
    res["pair"] = event_ms(lambda: rgbd_odometry_device(src, dst), a.reps)
    T, _, info = rgbd_odometry(src, dst)
    truth = np.linalg.inv(seq["poses"][0]) @ seq["poses"][1]
    res["pair"].update(n=info["n"], fitness=info["fitness"], translation_error_mm=float(1000 * np.linalg.norm(T[:3, 3] - truth[:3, 3])))
    track(seq["depth"][:3], color[:3], seq["K"])                                   # warm-up
    ev, wall = [], []
    for _ in range(a.track_reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        poses, kept = track(seq["depth"], color, seq["K"])
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    err = [float(np.linalg.norm((poses[f] - np.linalg.inv(seq["poses"][0]) @ seq["poses"][f])[:3, 3])) for f in range(a.frames)
           if kept[f]]
    res["track"] = dict(event_ms=dict(median=float(np.median(ev)), min=float(min(ev)), max=float(max(ev))),
                        wall_ms=dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall))),
                        reps=a.track_reps, kept=int(kept.sum()),
                        worst_translation_error_mm=float(1000 * max(err)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
