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


# ======================================================================================================================
# The inference block (csrc/fusion.hip: k_fusion_attn, then the two feed-forward GEMMs on the convolution kernels), from
# K / V on: tests/test_fusion_forward_host.py, tests/test_gpu_fusion_forward.py
# ======================================================================================================================
# name -> (rows per item, tokens per image, factor on to_q.weight)
FORWARD_SHAPES = {}
for _n in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97):       # the 16-row workgroup, 32 / 48 / 64-row GEMM units
    FORWARD_SHAPES[f"rows_{_n}"] = ((_n,), 300, 1.0)
for _rows in ((1, 16, 33), (31, 33), (48, 48, 1), (17, 5), (5, 17), (1,) * 8, (3, 64, 2, 47, 1, 16, 33, 15)):
    FORWARD_SHAPES["items_" + "_".join(map(str, _rows))] = (_rows, 300, 1.0)
for _t in (1, 63, 64, 65, 128, 129, 255, 256, 300, 320):                # 1 .. 20 column blocks of the score GEMM
    FORWARD_SHAPES[f"tokens_{_t}"] = ((17, 5), _t, 1.0)
for _t in (65, 300):                                                    # |score| near 87 and near 350
    for _f in (64.0, 256.0):
        FORWARD_SHAPES[f"softmax_t{_t}_x{int(_f)}"] = ((17,), _t, _f)
FORWARD_VARIANTS = (3, 0, 6)                                            # bf16x3 (the default), fp32 MFMA, split-f16
FORWARD_MODULE_SEED = 2000


def tokens_padded(T):
    return (T + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def forward_module(q_scale=1.0):
    """The one module of the forward catalogue (CPU fp32, default initialisation, noise on the LayerNorm parameters), with
    to_q.weight times `q_scale`."""
    with torch.random.fork_rng():
        torch.manual_seed(FORWARD_MODULE_SEED)
        module = new_module()
        g = torch.Generator().manual_seed(FORWARD_MODULE_SEED)
        with torch.no_grad():
            for key, p in module.named_parameters():
                if ".norm" in key:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
            module.cross_attend_blocks[0].fn.to_q.weight.mul_(q_scale)
    return module.eval()


def kv_of(module, tokens):
    """(k, v) [B, T, 128] fp32: to_kv(norm_context(tokens)) by torch on the tokens' device, K first."""
    blk = module.cross_attend_blocks[0]
    with torch.no_grad():
        k, v = blk.fn.to_kv(blk.norm_context(tokens)).chunk(2, dim=-1)
    return k.contiguous(), v.contiguous()


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """dict(rows, T, Tp, q_scale, starts, module, x [n, 256], k, v [B, T, 128]); all CPU fp32.  k / v are computed once,
    here: the packed images of the GPU, the restatement and the torch path all read these same values."""
    rows, T, q_scale = FORWARD_SHAPES[name]
    module = forward_module(q_scale)
    g = torch.Generator().manual_seed(3000 + sorted(FORWARD_SHAPES).index(name))
    n = sum(rows)
    x = torch.randn(n, 256, generator=g)
    tokens = torch.randn(len(rows), T, 128, generator=g)
    k, v = kv_of(module, tokens)
    starts = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return dict(rows=rows, T=T, Tp=tokens_padded(T), q_scale=q_scale, starts=starts, module=module, x=x, k=k, v=v)


@functools.lru_cache(maxsize=None)
def forward_reference(name):
    """z [n, 256] float64 of the restatement on the case's fp32 x, k, v."""
    c = forward_case(name)
    P = [w.numpy() for w in weights(c["module"])]
    return FR.forward_from_kv(c["x"].numpy(), c["starts"], c["k"].numpy(), c["v"].numpy(), P)[0]


def forward_torch_path(c, dtype=torch.float32, device="cpu"):
    """z of model/fusion.py's torch ops from the case's k / v on (ResUNet2._fusion_fast's sequence), item by item."""
    import copy
    import torch.nn.functional as F
    m = copy.deepcopy(c["module"]).to(device=device, dtype=dtype)
    blk0, blk1 = m.cross_attend_blocks
    att, ff = blk0.fn, blk1.fn.net
    x, k, v = (c[key].to(device=device, dtype=dtype) for key in ("x", "k", "v"))
    parts = []
    with torch.no_grad():
        for b in range(len(c["rows"])):
            xb = x[c["starts"][b]:c["starts"][b + 1]]
            q = F.linear(blk0.norm(xb), att.to_q.weight)
            p = torch.softmax((q @ k[b].t()) * att.scale, dim=-1)
            y = F.linear(p @ v[b], att.to_out.weight, att.to_out.bias) + xb
            h = F.linear(blk1.norm(y), ff[0].weight, ff[0].bias)
            a, gate = h.chunk(2, dim=-1)
            parts.append(F.linear(a * F.gelu(gate), ff[2].weight, ff[2].bias) + y)
    return torch.cat(parts, dim=0)


def item_errors(a, ref, starts):
    """[e(A) of each item's rows]: max|A - A64| / max|A64| over the item, so that a one-row item is not hidden behind a
    large one."""
    a = (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)
    return [float(np.abs(a[s:e] - ref[s:e]).max() / np.abs(ref[s:e]).max()) for s, e in zip(starts[:-1], starts[1:])]
