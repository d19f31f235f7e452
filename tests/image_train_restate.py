"""Float64 restatement of the image encoder's training step (csrc/image_train.hip, autograd.DenseConvFunction /
MaxPoolRowsFunction, model/image_encoder.py's kernel path): the yardstick of tests/test_image_train_host.py (which checks
it against torch's float64 autograd of the unchanged module) and tests/test_gpu_image_train.py.

  tables(B, H, W)        the six static pixel tables as integer arrays, the opposite ones built from the forward ones by
                         the relation nbrT[k][i] = o <=> nbr[k][o] = i
  maxpool_forward / maxpool_backward   3x3 / 2 / pad 1 on NHWC arrays, first maximum wins
  trunk(...)             forward and backward of conv1 .. layer2 in training mode on NHWC rows: every convolution as a sum
                         over the taps of a table, BatchNorm written out, the ReLU masks and the pool taps either its own
                         or the caller's (`decisions`)
Everything is NumPy or torch on the CPU in float64."""
import numpy as np
import torch
import torch.nn.functional as F

TILE, MASK_WORDS = 64, 4
TABLE_NAMES = ("t4", "t48", "t48T", "td", "tdT", "t8")


def trunk_shapes(H, W):
    down = lambda v, k, p: (v + 2 * p - k) // 2 + 1                         # noqa: E731
    h2, w2 = down(H, 7, 3), down(W, 7, 3)
    h4, w4 = down(h2, 3, 1), down(w2, 3, 1)
    return (h2, w2), (h4, w4), (down(h4, 3, 1), down(w4, 3, 1))


def _slots(n):
    return (n + TILE - 1) // TILE * TILE


def _mask_of(nbr, n_slots, force_tap0_rows=0):
    kvol = nbr.shape[0]
    mask = np.zeros((n_slots // TILE, MASK_WORDS), dtype=np.uint32)
    act = (nbr >= 0).reshape(kvol, n_slots // TILE, TILE).any(axis=2)
    if force_tap0_rows:
        act[0] |= (np.arange(n_slots) < force_tap0_rows).reshape(-1, TILE).any(axis=1)
    for k in range(kvol):
        mask[:, k // 32] |= (act[k].astype(np.uint32) << np.uint32(k % 32))
    return mask


def _finish(nbr, n_out, force_tap0=False):
    kvol, n_slots = nbr.shape
    rows = np.where(np.arange(n_slots) < n_out, np.arange(n_slots), -1).astype(np.int32)
    return dict(tile_rows=rows, nbr=nbr.astype(np.int32), tile_mask=_mask_of(nbr, n_slots, n_out if force_tap0 else 0),
                n_slots=n_slots, n_out=n_out, kvol=kvol)


def forward_table(B, Hin, Win, Hout, Wout, ksize, stride, pad):
    """rows = output pixels: nbr[k][o] = the input pixel o * stride + tap - pad, -1 outside the map or on a padding slot."""
    n_out = B * Hout * Wout
    nbr = np.full((ksize * ksize, _slots(n_out)), -1, dtype=np.int64)
    b, oy, ox = np.meshgrid(np.arange(B), np.arange(Hout), np.arange(Wout), indexing="ij")
    for k in range(ksize * ksize):
        iy, ix = oy * stride + k // ksize - pad, ox * stride + k % ksize - pad
        ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
        nbr[k, :n_out] = np.where(ok, (b * Hin + iy) * Win + ix, -1).reshape(-1)
    return _finish(nbr, n_out)


def opposite_table(fwd, n_rows, force_tap0=False):
    """rows = input pixels: nbrT[k][i] = o <=> nbr[k][o] = i (each input pixel is read through tap k by at most one output)."""
    nbr = np.full((fwd["kvol"], _slots(n_rows)), -1, dtype=np.int64)
    for k in range(fwd["kvol"]):
        o = np.nonzero(fwd["nbr"][k] >= 0)[0]
        i = fwd["nbr"][k][o]
        assert len(np.unique(i)) == len(i)
        nbr[k, i] = o
    return _finish(nbr, n_rows, force_tap0)


def tables(B, H, W):
    _, (h4, w4), (h8, w8) = trunk_shapes(H, W)
    t = dict(t4=forward_table(B, h4, w4, h4, w4, 3, 1, 1), t48=forward_table(B, h4, w4, h8, w8, 3, 2, 1),
             td=forward_table(B, h4, w4, h8, w8, 1, 2, 0), t8=forward_table(B, h8, w8, h8, w8, 3, 1, 1))
    t["t48T"] = opposite_table(t["t48"], B * h4 * w4)
    # tap 0 is marked active in every tile of tdT that holds a row: the convolution kernel skips tiles with an empty mask
    t["tdT"] = opposite_table(t["td"], B * h4 * w4, force_tap0=True)
    return t


# ---- max pool -------------------------------------------------------------------------------------------------------------
def maxpool_forward(x):
    """x [B, Hin, Win, C] -> (out, tap) [B, Hout, Wout, C]: taps inside the map in (ky, kx) order, a later one wins only
    when strictly greater; tap = ky * 3 + kx (uint8)."""
    x = np.asarray(x, dtype=np.float64)
    B, Hin, Win, C = x.shape
    Hout, Wout = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
    pad = np.full((B, 2 * Hout + 1, 2 * Wout + 1, C), -np.inf)
    pad[:, 1:Hin + 1, 1:Win + 1] = x
    inside = np.zeros((2 * Hout + 1, 2 * Wout + 1), dtype=bool)
    inside[1:Hin + 1, 1:Win + 1] = True
    oy, ox = np.meshgrid(np.arange(Hout), np.arange(Wout), indexing="ij")
    first = np.where(oy == 0, 3, 0) + np.where(ox == 0, 1, 0)
    m = np.full((B, Hout, Wout, C), -np.inf)
    t = np.broadcast_to(first[None, :, :, None], m.shape).astype(np.uint8).copy()
    for k in range(9):
        ky, kx = divmod(k, 3)
        v = pad[:, ky:ky + 2 * Hout:2, kx:kx + 2 * Wout:2]
        ok = inside[ky:ky + 2 * Hout:2, kx:kx + 2 * Wout:2][None, :, :, None]
        take = ok & (v > m)
        m = np.where(take, v, m)
        t = np.where(take, np.uint8(k), t)
    return m, t


def maxpool_backward(dout, tap, Hin, Win):
    """din [B, Hin, Win, C]: dout goes to the pixel its window's tap points at (exact sums in float64)."""
    dout = np.asarray(dout, dtype=np.float64)
    B, Hout, Wout, C = dout.shape
    pad = np.zeros((B, 2 * Hout + 1, 2 * Wout + 1, C))
    for k in range(9):
        ky, kx = divmod(k, 3)
        pad[:, ky:ky + 2 * Hout:2, kx:kx + 2 * Wout:2] += np.where(tap == k, dout, 0.0)   # one window per pixel and tap
    return pad[:, 1:Hin + 1, 1:Win + 1].copy()


def maxpool_select(x, tap):
    """out [B, Hout, Wout, C] = the value of x [B, Hin, Win, C] each window's `tap` points at."""
    x = np.asarray(x, dtype=np.float64)
    B, Hin, Win, C = x.shape
    Hout, Wout = tap.shape[1:3]
    pad = np.zeros((B, 2 * Hout + 1, 2 * Wout + 1, C))
    pad[:, 1:Hin + 1, 1:Win + 1] = x
    out = np.zeros(tap.shape)
    for k in range(9):
        ky, kx = divmod(k, 3)
        out = np.where(tap == k, pad[:, ky:ky + 2 * Hout:2, kx:kx + 2 * Wout:2], out)
    return out


class _Pool(torch.autograd.Function):
    """The pool with its decisions given: forward selects, backward routes."""

    @staticmethod
    def forward(ctx, x, tap):
        ctx.tap, ctx.hw = tap, x.shape[1:3]
        return torch.from_numpy(np.ascontiguousarray(maxpool_select(x.detach().numpy(), tap)))

    @staticmethod
    def backward(ctx, g):
        return torch.from_numpy(maxpool_backward(g.numpy(), ctx.tap, *ctx.hw)), None


# ---- the trunk ------------------------------------------------------------------------------------------------------------
def im2col7(image):
    """[B,3,H,W] -> [B*H2*W2, 160]: column (ky*7+kx)*3 + ch, columns 147..159 zero."""
    B = image.shape[0]
    u = F.unfold(image, 7, padding=3, stride=2)               # [B, ch*49 + ky*7 + kx, L]
    u = u.view(B, 3, 49, -1).permute(0, 3, 2, 1).reshape(-1, 147)
    return torch.cat([u, u.new_zeros((u.shape[0], 13))], dim=1)


def table_conv(x, weight, table):
    """out[o] = sum_k x[nbr[k][o]] @ W[k] with W[k][ci][co] = weight[co][ci][ky][kx]."""
    co, ci, kh, kw = weight.shape
    k3 = weight.permute(2, 3, 1, 0).reshape(kh * kw, ci, co)
    xz = torch.cat([x, x.new_zeros((1, ci))])                 # index -1 -> the zero row
    out = x.new_zeros((table["n_out"], co))
    for k in range(table["kvol"]):
        idx = torch.from_numpy(table["nbr"][k][: table["n_out"]].astype(np.int64))
        out = out + xz[idx] @ k3[k]
    return out


def conv_names():
    """(convolution, norm) parameter prefixes below `backbone.` in execution order: 16 pairs."""
    names = [("conv1", "bn1")]
    for layer, blocks in (("layer1", 3), ("layer2", 4)):
        for i in range(blocks):
            names.append((f"{layer}.{i}.conv1", f"{layer}.{i}.bn1"))
            if layer == "layer2" and i == 0:
                names.append((f"{layer}.{i}.downsample.0", f"{layer}.{i}.downsample.1"))
            names.append((f"{layer}.{i}.conv2", f"{layer}.{i}.bn2"))
    return names


def grad_names():
    return [f"backbone.{c}.weight" for c, _ in conv_names()] + [f"backbone.{n}.{p}" for _, n in conv_names()
                                                                  for p in ("weight", "bias")]


def stat_names():
    return [f"backbone.{n}.{p}" for _, n in conv_names() for p in ("running_mean", "running_var")]


def trunk(state, image, grad_out, decisions=None, momentum=0.1, eps=1e-5):
    """One training-mode forward and backward.  state: the module's state_dict; image [B,3,H,W]; grad_out [B,128,H8,W8].
    decisions: the list the kernel path's `trace` gives (ReLU outputs or masks, and the pool's taps as [rows, C]), used
    instead of the trunk's own.  Returns dict(out [B,128,H8,W8], grads {name: array}, stats {name: array},
    decisions [15 ReLU masks and the taps in execution order, as boolean / uint8 arrays of rows])."""
    sd = {k: torch.as_tensor(np.asarray(v, dtype=np.float64) if not torch.is_tensor(v) else v.detach().cpu().double().numpy())
          for k, v in state.items() if k.startswith("backbone.") and not k.endswith("num_batches_tracked")}
    params = {k: sd[k].clone().requires_grad_(True) for k in grad_names()}
    image = torch.as_tensor(image).detach().cpu().double()
    B, _, H, W = image.shape
    (h2, w2), (h4, w4), (h8, w8) = trunk_shapes(H, W)
    T = tables(B, H, W)
    forced = None if decisions is None else list(decisions)
    taken, stats = [], {}

    def norm(x, name, residual, relu):
        n = x.shape[0]
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        y = (x - mean) / torch.sqrt(var + eps) * params[f"backbone.{name}.weight"] + params[f"backbone.{name}.bias"]
        with torch.no_grad():
            stats[f"backbone.{name}.running_mean"] = ((1 - momentum) * sd[f"backbone.{name}.running_mean"] + momentum * mean).numpy()
            stats[f"backbone.{name}.running_var"] = ((1 - momentum) * sd[f"backbone.{name}.running_var"]
                                                     + momentum * var * n / (n - 1)).numpy()
        if residual is not None:
            y = y + residual
        if relu:
            if forced is None:
                mask = y.detach() > 0
            else:
                d = forced[len(taken)]
                mask = torch.as_tensor(d).detach().cpu() > 0
            taken.append(mask.numpy())
            y = y * mask
        return y

    w = lambda name: params[f"backbone.{name}.weight"]                       # noqa: E731
    stem_w = torch.cat([w("conv1").permute(2, 3, 1, 0).reshape(147, 64), torch.zeros((13, 64), dtype=torch.float64)])
    y = norm(im2col7(image) @ stem_w, "bn1", None, True)
    if forced is None:
        tap = maxpool_forward(y.detach().numpy().reshape(B, h2, w2, 64))[1]
    else:
        tap = torch.as_tensor(forced[len(taken)]).cpu().numpy().reshape(B, h4, w4, 64)
    taken.append(tap.reshape(B * h4 * w4, 64))
    y = _Pool.apply(y.view(B, h2, w2, 64), tap).reshape(B * h4 * w4, 64)
    for layer, blocks, t_same in (("layer1", 3, T["t4"]), ("layer2", 4, T["t8"])):
        for i in range(blocks):
            p = f"{layer}.{i}"
            strided = layer == "layer2" and i == 0
            z = norm(table_conv(y, w(f"{p}.conv1"), T["t48"] if strided else t_same), f"{p}.bn1", None, True)
            z = table_conv(z, w(f"{p}.conv2"), t_same)
            if strided:
                y = norm(table_conv(y, w(f"{p}.downsample.0"), T["td"]), f"{p}.downsample.1", None, False)
            y = norm(z, f"{p}.bn2", y, True)
    out = y.view(B, h8, w8, 128).permute(0, 3, 1, 2)
    g = torch.as_tensor(grad_out).detach().cpu().double()
    names = grad_names()
    grads = torch.autograd.grad(out, [params[k] for k in names], g)
    return dict(out=out.detach().numpy().copy(), grads={k: v.numpy() for k, v in zip(names, grads)}, stats=stats,
                decisions=taken)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def seeded_encoder(seed, dtype=torch.float32):
    """ImageEncoder with its default initialisation under `seed`, then gamma ~ U(0.5, 1.5) and beta ~ U(-0.1, 0.1) on
    every BatchNorm (the default 1 / 0 would leave most of the backward's terms untested)."""
    from imfnet_amd.model.image_encoder import ImageEncoder
    gen = torch.Generator().manual_seed(1000 + seed)
    torch.manual_seed(seed)
    enc = ImageEncoder()
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=gen) * 0.2 - 0.1)
    return enc.to(dtype)


def seeded_inputs(B, H, W, seed):
    """(image in [0, 1) [B,3,H,W], Gaussian grad_out [B,128,H8,W8]) as float32 tensors."""
    gen = torch.Generator().manual_seed(2000 + seed)
    _, _, (h8, w8) = trunk_shapes(H, W)
    return torch.rand((B, 3, H, W), generator=gen), torch.randn((B, 128, h8, w8), generator=gen)


def rel_err(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    return float(np.abs(a - ref).max()) / scale if scale > 0 else float(np.abs(a).max())


def module_step(enc, image, grad_out, trace=None):
    """One forward and backward of an ImageEncoder module (any dtype / device / switch): dict(out, grads, stats) as
    float64 arrays; the module's running statistics move."""
    enc.train()
    enc.zero_grad(set_to_none=True)
    out = enc(image) if trace is None else enc(image, trace=trace)
    out.backward(grad_out)
    named = dict(enc.named_parameters())
    sd = enc.state_dict()
    return dict(out=out.detach().cpu().double().numpy(),
                grads={k: named[k].grad.detach().cpu().double().numpy() for k in grad_names()},
                stats={k: sd[k].detach().cpu().double().numpy() for k in stat_names()})
