"""The inputs both fusion-training test files use (tests/test_fusion_train_host.py, tests/test_gpu_fusion_train.py): the
shapes, the seeded module and tensors, the torch path of model/fusion.py run item by item as ResUNet2.transformer runs it,
and the float64 restatement's outputs, computed once per case."""
import functools

import numpy as np
import torch

import fusion_restate as FR

CHUNK = 256                       # imf_fusion_train_chunk_rows(); test_fusion_train_host.py checks the library agrees
# name -> (rows per item, tokens per image)
SHAPES = {
    "rows_1": ((1,), 300),
    "rows_15": ((15,), 300),
    "rows_16": ((16,), 300),
    "rows_17": ((17,), 300),
    "rows_1_16_33": ((1, 16, 33), 300),
    "rows_40_0_7": ((40, 0, 7), 300),
    "two_chunks_and_a_row": ((2 * CHUNK + 1,), 300),
    "tokens_65": ((17, 5), 65),
}
PARAMS = (
    "cross_attend_blocks.0.norm.weight", "cross_attend_blocks.0.norm.bias",
    "cross_attend_blocks.0.norm_context.weight", "cross_attend_blocks.0.norm_context.bias",
    "cross_attend_blocks.0.fn.to_q.weight", "cross_attend_blocks.0.fn.to_kv.weight",
    "cross_attend_blocks.0.fn.to_out.weight", "cross_attend_blocks.0.fn.to_out.bias",
    "cross_attend_blocks.1.norm.weight", "cross_attend_blocks.1.norm.bias",
    "cross_attend_blocks.1.fn.net.0.weight", "cross_attend_blocks.1.fn.net.0.bias",
    "cross_attend_blocks.1.fn.net.2.weight", "cross_attend_blocks.1.fn.net.2.bias",
)
TENSORS = ("z", "dx", "dtokens") + PARAMS


def new_module():
    from imfnet_amd.model.fusion import AttentionFusion
    return AttentionFusion(dim=128, depth=0, latent_dim=256, cross_heads=1, latent_heads=8, cross_dim_head=128,
                           latent_dim_head=128)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(rows, T, starts, module (CPU fp32, default initialisation, LayerNorm parameters with noise), x, tokens, dz)."""
    rows, T = SHAPES[name]
    seed = 1000 + sorted(SHAPES).index(name)
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        module = new_module()
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for key, p in module.named_parameters():
                if ".norm" in key:                       # gamma != 1, beta != 0
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        n = sum(rows)
        x = torch.randn(n, 256, generator=g)
        tokens = torch.randn(len(rows), T, 128, generator=g)
        dz = torch.randn(n, 256, generator=g)
    starts = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return dict(rows=rows, T=T, starts=starts, module=module, x=x, tokens=tokens, dz=dz)


def weights(module, device=None, dtype=None):
    sd = dict(module.named_parameters())
    return [sd[k].detach().to(device=device, dtype=dtype).contiguous() for k in PARAMS]


def torch_path(c, dtype=torch.float32, device="cpu"):
    """{tensor name: result} of model/fusion.py's torch ops under torch's autograd, item by item as
    ResUNet2.transformer's torch body runs them, in `dtype` on `device`."""
    import copy
    m = copy.deepcopy(c["module"]).to(device=device, dtype=dtype)
    x = c["x"].to(device=device, dtype=dtype).requires_grad_(True)
    tokens = c["tokens"].to(device=device, dtype=dtype).requires_grad_(True)
    parts, start = [], 0
    for b, n in enumerate(c["rows"]):
        parts.append(m(tokens[b:b + 1], queries_encoder=x[start:start + n].unsqueeze(0))[0])
        start += n
    z = torch.cat(parts, dim=0)
    z.backward(c["dz"].to(device=device, dtype=dtype))
    out = {"z": z.detach(), "dx": x.grad, "dtokens": tokens.grad}
    out.update({k: p.grad for k, p in m.named_parameters()})
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """{tensor name: float64 array} of the restatement on the case's fp32 inputs."""
    c = case(name)
    P = [w.numpy() for w in weights(c["module"])]
    z, cache = FR.forward(c["x"].numpy(), c["starts"], c["tokens"].numpy(), P)
    dx, dtok, G = FR.backward(c["dz"].numpy(), cache)
    out = {"z": z, "dx": dx, "dtokens": dtok}
    out.update(dict(zip(PARAMS, G)))
    return out


def rel_err(a, ref):
    """e(A) = max|A - A64| / max|A64|."""
    a = (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)
    return float(np.abs(a.reshape(ref.shape) - ref).max() / np.abs(ref).max())
