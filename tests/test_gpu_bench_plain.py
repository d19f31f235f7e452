"""A plain `bench.py` run (no --full): the headline only -- ONE timed region of exactly --steps steps, no roofline, no legs,
no side file -- and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    import bench
    import imf_oracle_cbind as OC
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--settle-ms", "50",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    c = json.loads(r.stdout.splitlines()[-1])
    assert c["steps"] == 7 and c["warmup"] == 2 and c["timing"]["repeats"] == 1
    assert c["unit"] == "descriptors/s" and c["higher_is_better"] is True and c["dtype"] == "f32 (bf16x3)"
    assert c["ms_per_step"] > 0 and c["value"] > 0
    assert c["roofline"] is None and c["cpu_baseline"] is None and c["host_span"] is None and c["full_record"] is None

    F, xd = np.load(out / "descriptors.npy"), np.load(out / "xyz_down.npy")
    M = c["config"]["voxels_per_step_per_gpu"]
    assert sorted(os.listdir(out)) == ["descriptors.npy", "xyz_down.npy"]
    assert F.dtype == np.float32 and F.shape == (M, 32) and xd.dtype == np.float64 and xd.shape == (M, 3)
    pts, imgs = bench.load_pair(1.7)                                    # the default workload: the pair, one forward
    ref = np.concatenate([p[OC.voxelize(p, 0.025)[1]] for p in pts])
    assert (xd == ref).all()
    # the descriptors of the exact path on the same inputs (test_gpu_harness pins that path to the oracle), bit for bit
    dev = torch.device("cuda:0")
    model, _ = bench.build_model(dev)
    with torch.no_grad():
        F_exact = bench.Workload(model, dev, pts, imgs, 0.025).exact_step()
        torch.cuda.synchronize()                                        # (computed on the workload's own stream)
    assert (F == F_exact.cpu().numpy()).all()
