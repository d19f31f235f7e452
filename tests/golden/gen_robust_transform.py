#!/usr/bin/env python3
"""Generates tests/golden/robust_transform.npz.  Runs ONLY where the reference checkout is present; the tests use
the .npz file.

For every case of tests/robust_restate.py (six families, three seeds each) it stores pts1 of the float32
correspondence set (as int16 multiples of the family's power-of-two grid, which is exact; pts0 and the explicit
weights come from robust_restate's integer counter generator and are rebuilt on load, exactly),
the result of the reference's own est_quad_linear_robust on it (util/transform_estimation.py, imported over an empty
stand-in for MinkowskiEngine; pure torch, float32, CPU), and what float32 costs upstream: gap_R = max|R_up - R_64| and
gap_t = max|t_up - t_64| against the fp64 NumPy restatement of the same 20 rounds.  Also stored for the record:
how far upstream's result is from the planted motion.  No reference source text is copied; only inputs and numeric
outputs are stored.  A case whose gap exceeds 1e-4 is ill conditioned and stops the generator."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
import robust_restate as RR  # noqa: E402


def upstream():
    sys.modules.setdefault("MinkowskiEngine", types.ModuleType("MinkowskiEngine"))
    spec = importlib.util.spec_from_file_location("ref_transform_estimation",
                                                  os.path.join(REF, "util", "transform_estimation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.est_quad_linear_robust


def main():
    torch.set_num_threads(8)
    est = upstream()
    out = {}
    for fam, kw in RR.FAMILIES.items():
        for seed in RR.SEEDS:
            p0, p1, w, planted = RR.make_case(seed=seed, **kw)
            Tw = None if w is None else torch.from_numpy(w).reshape(-1, 1)
            T_up = est(torch.from_numpy(p0), torch.from_numpy(p1), Tw).numpy().astype(np.float32)
            T64 = RR.robust_transform_f64(p0, p1, w)
            gap_R = float(np.abs(T_up[:3, :3].astype(np.float64) - T64[:3, :3]).max())
            gap_t = float(np.abs(T_up[:3, 3].astype(np.float64) - T64[:3, 3]).max())
            dt = float(np.linalg.norm(T_up[:3, 3] - planted[:3, 3]))
            cosv = (np.trace(T_up[:3, :3].astype(np.float64).T @ planted[:3, :3]) - 1) / 2
            ddeg = float(np.rad2deg(np.arccos(np.clip(cosv, -1, 1))))
            print(f"{fam} seed {seed}: gap_R {gap_R:.2e} gap_t {gap_t:.2e}; upstream vs planted {dt * 1e3:.1f} mm "
                  f"{ddeg:.3f} deg")
            if max(gap_R, gap_t) > 1e-4:
                raise SystemExit(f"{fam} seed {seed} is ill conditioned: replace the case")
            k = f"{fam}_{seed}_"
            for name, pts in (("pts1_q", p1),):                         # int16 multiples of the grid, exact
                q = np.round(pts.astype(np.float64) / kw["grid"])
                assert np.abs(q).max() < 32768 and np.array_equal(q.astype(np.int16).astype(np.float32)
                                                                  * np.float32(kw["grid"]), pts)
                out[k + name] = q.astype(np.int16)
            out[k + "T_upstream"] = T_up
            out[k + "gap_R"], out[k + "gap_t"] = np.float64(gap_R), np.float64(gap_t)
            out[k + "planted"] = planted
    path = os.path.join(HERE, "robust_transform.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
