"""The training step of the InstanceNorm family gives the same gradient bits twice: the gate of
tests/test_gpu_train_repro.py with `--model ResUNetIN2C`.  One hardest-contrastive step on the fixture pair as a batch of
two, all six kernel switches at `hip`, run twice in one process from the same seed (imfnet_amd/train/repro.py).  Every
parameter's gradient must be torch.equal between the runs, or None in both, and the logged losses equal as Python floats.
With `--norm_kernels hip` the fourteen block norms run on the imf_in_* kernels: no index_add_ atomics are left in the
step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_one_step_of_resunet_in2c_with_all_six_switches_at_hip_gives_the_same_gradient_bits_twice(tmp_path, clouds, images,
                                                                                                  monkeypatch):
    from imfnet_amd import ops
    from imfnet_amd.autograd import SparseInstanceNormFunction as Fn
    from imfnet_amd.train import repro
    thin = {k: np.asarray(clouds[k])[::3] for k in (0, 1)}
    hwc = {k: np.transpose(np.asarray(images[k])[0], (1, 2, 0)) for k in (0, 1)}
    repro.write_tree(str(tmp_path), thin, hwc)
    calls, inner = [], Fn.forward

    def counted(ctx, *a):
        calls.append(1)
        return inner(ctx, *a)
    monkeypatch.setattr(Fn, "forward", staticmethod(counted))
    prev = (ops.TRAIN_NORM, ops.TRAIN_LOSS, ops.TRAIN_FUSION, ops.TRAIN_IMAGE, ops.TRAIN_OPTIM, ops.TRAIN_HEAD)
    try:
        res = repro.compare(str(tmp_path), 2, "hip", extra_args=("--model", "ResUNetIN2C"))
        assert (ops.TRAIN_NORM, ops.TRAIN_LOSS, ops.TRAIN_FUSION, ops.TRAIN_IMAGE, ops.TRAIN_OPTIM, ops.TRAIN_HEAD) == ("hip",) * 6
    finally:
        for setter, value in zip((ops.set_train_norm, ops.set_train_loss, ops.set_train_fusion, ops.set_train_image,
                                  ops.set_train_optim, ops.set_train_head), prev):
            setter(value)
    print({k: res[k] for k in ("parameters", "agree", "no_gradient", "groups", "loss_a", "loss_b")})
    # two fragments per pair and two runs: 2 * 2 * 14 block norms, every one of them on the HIP op
    assert len(calls) == 56
    assert res["parameters"] > 100 and res["parameters"] - res["no_gradient"] > 100
    assert all(np.isfinite(res["loss_a"])) and res["loss_a"][0] > 0
    differing_groups = {g: v for g, v in res["groups"].items() if v["agree"] != v["parameters"]}
    assert not res["differing"], (differing_groups, [d["name"] for d in res["differing"]])
    assert res["agree"] == res["parameters"]
    assert all(isinstance(v, float) for v in res["loss_a"] + res["loss_b"])
    assert res["loss_a"] == res["loss_b"] and res["loss_bits_agree"]
