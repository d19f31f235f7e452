"""`FusedSGD`: torch.optim.SGD whose step is ONE launch of the library (csrc/optim.hip, imf_sgd_step) over every parameter
(python -m imfnet_amd.train --optim_kernels hip, ops.TRAIN_OPTIM == "hip").

A subclass of torch.optim.SGD: `param_groups`, `state_dict()` / `load_state_dict()` with `momentum_buffer`, the learning
rate schedulers and the checkpoint format are torch's; a checkpoint of either optimizer resumes under the other.  Only
what the trainer uses is implemented -- one parameter group, dampening 0, no Nesterov, not maximising; everything else is
refused with an ImfError.  The arithmetic is torch's per element in fp32 with every operation rounded once (the header of
csrc/optim.hip), bit for bit a function of (p, g, b, lr, momentum, weight_decay).

With a `model`, the launch also writes the two bf16x3 operand images of every packable convolution weight it updates
(cin % 32 == 0, cout % 32 == 0, kvol <= 27, training arithmetic bf16x3): the sparse convolutions' kernels, and with
ops.TRAIN_IMAGE == "hip" the 15 dense convolutions the image encoder's kernel path runs.  ops.weight_image hands them to
the differentiable convolutions (autograd.py) while the parameter's `_version` is the one this step left, so an iteration
packs no weight this optimizer owns; a parameter with images is also watched for `.data` accesses, which no version counter
sees (ops._WatchedParameter).  Every written parameter's `_version` is incremented (the step writes through raw
pointers): the inference caches keyed on it (sparse.py `packed()`, the packed model of the runner) see the change.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from .. import _lib, ops
from .._lib import ImfError, check


def _record_dtype():
    """numpy view of _lib.SgdRecord (pointers as unsigned integers)."""
    names, formats, offsets = [], [], []
    for name, ctype in _lib.SgdRecord._fields_:
        names.append(name)
        formats.append("<u8" if ctype is C.c_void_p else np.dtype(ctype).str)
        offsets.append(getattr(_lib.SgdRecord, name).offset)
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=C.sizeof(_lib.SgdRecord)))


def packable(kvol, cin, cout):
    """Whether a convolution weight gets operand images from the step: the shapes the bf16x3 image exists for."""
    from ..autograd import training_variant
    return cin % 32 == 0 and cout % 32 == 0 and 1 <= kvol <= ops.MAX_PIPELINED_KVOL and training_variant(kvol) == 3


def conv_records(model):
    """{id(parameter): (layout, kvol, cin, cout, flip, wants the backward image)} of the model's packable convolution
    weights: every sparse convolution's kernel (ME layout; flip iff not transposed and stride 1, the rule of
    autograd.SparseConvFunction; no backward image for kvol == 1, whose input gradient is a matrix product), and with
    ops.TRAIN_IMAGE == "hip" the image encoder's executed convolutions (torch layout, flip as its training forward passes
    it to autograd.DenseConvFunction).  Empty under fp32 arithmetic (ops.CONV_VARIANT == 0): no image is built."""
    from .. import sparse
    from ..autograd import conv_flips_taps
    from ..model.image_encoder import ImageEncoder
    out = {}
    for m in model.modules():
        if isinstance(m, sparse._ConvBase) and packable(m.kernel_volume, m.in_channels, m.out_channels):
            out[id(m.kernel)] = (_lib.SGD_ME, m.kernel_volume, m.in_channels, m.out_channels, conv_flips_taps(m),
                                 m.kernel_volume > 1)
        elif isinstance(m, ImageEncoder) and ops.TRAIN_IMAGE == "hip":
            for conv, flip in m.executed_convs():
                co, ci, kh, kw = conv.weight.shape
                if packable(kh * kw, ci, co):
                    out[id(conv.weight)] = (_lib.SGD_TORCH, kh * kw, ci, co, bool(flip), True)
    return out


def _drop_images(entries):
    for ent in entries:
        ops.unregister_weight_images(ent)


class FusedSGD(torch.optim.SGD):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 model=None, convs=None, **kwargs):
        """`model`: the module whose convolution weights get operand images (conv_records); `convs`: such a table given
        directly, {id(parameter): (layout, kvol, cin, cout, flip, backward image)}.  Neither: an element-wise step only."""
        self._refuse(dampening, nesterov, maximize)
        self._convs = dict(convs or {})
        if model is not None:
            self._convs.update(conv_records(model))
        self._table = None
        self._images = {}                      # id(parameter) -> ops.WeightImages
        self._upload_done = self._finalizer = self._map_key = None
        self._maps = {}                        # tuple of active record indices -> (block map, n_blocks)
        super().__init__(params, lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False,
                         maximize=False, **kwargs)
        if all(p.is_cuda for p in self.param_groups[0]["params"]):
            self._prepare()

    @staticmethod
    def _refuse(dampening, nesterov, maximize):
        if dampening != 0:
            raise ImfError(f"FusedSGD: dampening={dampening} is not implemented (0 only)")
        if nesterov:
            raise ImfError("FusedSGD: Nesterov momentum is not implemented")
        if maximize:
            raise ImfError("FusedSGD: maximize is not implemented")

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ImfError("FusedSGD: one parameter group only")
        super().add_param_group(param_group)

    # ---- tables ----------------------------------------------------------------------------------------------------
    def _prepare(self):
        """The static half: the record table (pinned and device), the image arena and the images of the weights as they
        are now."""
        params = self.param_groups[0]["params"]
        dev = params[0].device
        chunk = _lib.lib().imf_sgd_chunk()
        dt = _record_dtype()
        n = len(params)
        blocks = sum(-(-p.numel() // chunk) for p in params)
        map_off = (n * dt.itemsize + 255) // 256 * 256
        nbytes = map_off + max(blocks, 1) * 8
        self._pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self._device = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        host = self._pinned.numpy()
        host[:] = 0
        self._rec = host[:n * dt.itemsize].view(dt)
        self._map = host[map_off:map_off + max(blocks, 1) * 8].view(np.int32).reshape(-1, 2)
        self._map_off, self._chunk, self._params = map_off, chunk, list(params)
        self._chunks = [-(-p.numel() // chunk) for p in params]
        # images: one arena, every image on a 256-byte boundary
        sizes, total = {}, 0
        for i, p in enumerate(params):
            spec = self._convs.get(id(p))
            if spec is None or not (p.is_cuda and p.dtype == torch.float32):
                continue
            layout, kvol, cin, cout, flip, bwd = spec
            # the kernel trusts its records: everything it indexes with is checked here
            shape = ((cout, cin) if layout == _lib.SGD_TORCH else ((kvol, cin, cout) if p.dim() == 3 else (cin, cout)))
            if (layout not in (_lib.SGD_ME, _lib.SGD_TORCH) or cin <= 0 or cout <= 0 or cin % 32 or cout % 32 or
                    not 1 <= kvol <= ops.MAX_PIPELINED_KVOL or p.numel() != kvol * cin * cout or
                    tuple(p.shape[:len(shape)]) != shape or not p.is_contiguous()):
                raise ImfError(f"FusedSGD: parameter {i} {tuple(p.shape)} is no packable [{kvol}, {cin}, {cout}] kernel "
                               f"of layout {layout}")
            need = (p.numel() * 3 // 2 + 63) // 64 * 64
            sizes[i] = (total, total + need if bwd else None, p.numel() * 3 // 2)
            total += need * (2 if bwd else 1)
        self._arena = torch.empty(total, dtype=torch.float32, device=dev) if total else None
        _drop_images(self._images.values())
        if self._finalizer is not None:
            self._finalizer.detach()
        self._images, self._maps, self._map_key = {}, {}, None
        rec = self._rec
        for i, p in enumerate(params):
            rec["numel"][i] = p.numel()
            if i not in sizes:
                rec["layout"][i] = _lib.SGD_PLAIN
                continue
            layout, kvol, cin, cout, flip, bwd = self._convs[id(p)]
            f0, b0, need = sizes[i]
            fwd = self._arena[f0:f0 + need]
            back = self._arena[b0:b0 + need] if bwd else None
            rec["layout"][i], rec["kvol"][i], rec["cin"][i], rec["cout"][i], rec["flip"][i] = layout, kvol, cin, cout, int(flip)
            rec["image_fwd"][i], rec["image_bwd"][i] = fwd.data_ptr(), (back.data_ptr() if bwd else 0)
            ent = ops.WeightImages(p, fwd, back, flip)
            ops.pack_weights(ops.image_source(p, "forward"), out=fwd, variant=3)
            if bwd:
                ops.pack_weights(ops.image_source(p, "backward", flip), out=back, variant=3)
            ent.version = p._version
            ops.register_weight_images(p, ent)
            self._images[id(p)] = ent
        self._finalizer = weakref.finalize(self, _drop_images, list(self._images.values()))
        self._table = True

    def images(self, param):
        """(forward image, backward image or None) this optimizer keeps for `param`, or None when it keeps none."""
        ent = self._images.get(id(param))
        return None if ent is None else (ent.fwd, ent.bwd)

    def image_bytes(self):
        """Device bytes of the image arena (about 3 x the fp32 size of the packable weights: two images of 1.5 x each)."""
        return 0 if self._table is None or self._arena is None else self._arena.numel() * 4

    # ---- the step --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise ImfError("FusedSGD: one parameter group only")
        group = self.param_groups[0]
        self._refuse(group["dampening"], group["nesterov"], group["maximize"])
        params = group["params"]
        mu, wd, lr = float(group["momentum"]), float(group["weight_decay"]), float(group["lr"])
        if self._table is None or len(params) != len(self._params) or any(a is not b for a, b in zip(params, self._params)):
            if not all(p.is_cuda for p in params):
                raise ImfError("FusedSGD: parameters must be CUDA(HIP) tensors -- imfnet_amd has no CPU path")
            self._prepare()
        active, p_ptr, g_ptr, b_ptr, first, keep = [], [], [], [], [], []
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                continue
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ImfError(f"FusedSGD: parameter {i} must be a contiguous fp32 CUDA(HIP) tensor")
            if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                raise ImfError(f"FusedSGD: the gradient of parameter {i} must be a dense fp32 tensor of its shape and device")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            buf, new = None, False
            if mu != 0:
                state = self.state[p]
                buf = state.get("momentum_buffer")
                if buf is None:
                    buf = state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    new = True
                elif not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.shape == p.shape):
                    raise ImfError(f"FusedSGD: the momentum buffer of parameter {i} must be a contiguous fp32 tensor of its shape")
            active.append(i)
            p_ptr.append(p.data_ptr())
            g_ptr.append(g.data_ptr())
            b_ptr.append(0 if buf is None else buf.data_ptr())
            first.append(int(new))
        if not active:
            return loss
        if self._upload_done is not None:
            self._upload_done.synchronize()           # the last step's copy has read the pinned table
        rec = self._rec
        rec["param"][active], rec["grad"][active], rec["momentum"][active], rec["first_step"][active] = p_ptr, g_ptr, b_ptr, first
        key = tuple(active)
        cached = self._maps.get(key)
        if cached is None:
            rows = np.concatenate([np.stack([np.full(self._chunks[i], i, np.int32), np.arange(self._chunks[i], dtype=np.int32)], 1)
                                   for i in active])
            self._maps = {key: rows}
            cached = rows
        if self._map_key != key:
            self._map[:len(cached)] = cached
            self._map_key = key
        self._device.copy_(self._pinned, non_blocking=True)
        self._upload_done = torch.cuda.Event()
        self._upload_done.record()
        base = self._device.data_ptr()
        check(_lib.lib().imf_sgd_step(base, len(params), base + self._map_off, len(cached), lr, mu, wd,
                                      torch.cuda.current_stream().cuda_stream), "imf_sgd_step")
        written = [params[i] for i in active]
        torch.autograd.graph.increment_version(written)
        for p in written:
            ent = self._images.get(id(p))
            if ent is not None:
                ent.version = p._version
                if ent.key != p.data_ptr():           # the parameter moved (module.to(...)): found under its new address
                    ops.unregister_weight_images(ent)
                    ops.register_weight_images(p, ent)
        return loss

