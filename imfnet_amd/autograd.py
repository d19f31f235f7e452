"""Training backward of the sparse convolutions (last item; the reference trains through
MinkowskiEngine's autograd, lib/trainer.py:495-569).

`SparseConvFunction` wraps one ME.MinkowskiConvolution / ConvolutionTranspose:
  forward   imf_spconv_fwd (the inference kernel, no fused epilogue -- BatchNorm / ReLU / residual stay torch ops in
            training mode, so their gradients are torch's);
  d input   imf_spconv_fwd again over the OPPOSITE kernel map with transposed weights:
              stride 1      the same map, W'[k] = W[K-1-k]^T          (offsets are symmetric: off[K-1-k] = -off[k])
              stride 2      the transposed map coarse -> fine, W'[k] = W[k]^T
              transposed    the strided map fine -> coarse, W'[k] = W[k]^T
              1x1x1         grad @ W^T
  d kernel  imf_spconv_wgrad (csrc/backward.hip): per offset the sum of in[i]^T grad[o] over the map's pairs.
Everything stays on the GPU; the maps come from the coordinate manager's cache (built once per fragment).

`SparseBatchNormFunction` is the training-mode BatchNorm between them (csrc/norm_train.hip, ops.TRAIN_NORM == "hip"):
fp64 batch statistics in a fixed order, the ReLU and the residual add of the residual block folded in, forward and
backward; sparse.MinkowskiBatchNorm decides when it runs.  `SparseInstanceNormFunction` is the same for the InstanceNorm of
the ResUNetIN2* residual blocks, the statistics cut per batch item over a device-side partition of the rows;
sparse.MinkowskiInstanceNorm decides when it runs.

`HardestContrastiveLossFunction` is the loss at the end (csrc/loss.hip, ops.TRAIN_LOSS == "hip"): both losses, the
hardest negatives and the closed-form gradient with respect to the two feature matrices, fp64 sums in a fixed order;
train.loss.hardest_contrastive_loss decides when it runs.

`AttentionFusionFunction` is the bottleneck point <-> image attention block (csrc/fusion_train.hip, ops.TRAIN_FUSION ==
"hip"): every batch item in one forward and one backward call over a device-side partition of the rows;
ResUNet2.transformer decides when it runs.

`DenseConvFunction` / `MaxPoolRowsFunction` are the image encoder's convolutions and max pool on NHWC rows
(csrc/image_train.hip, ops.TRAIN_IMAGE == "hip"): the same three kernels as `SparseConvFunction` over static pixel tables,
`SparseBatchNormFunction` between them; model.image_encoder.ImageEncoder decides when they run.

`HeadFunction` is the descriptor head at the end of the decoder (csrc/head_train.hip, ops.TRAIN_HEAD == "hip"): the
concatenation with the stride-1 skip, conv1_tr, ReLU, final and the L2 normalisation as one forward and one backward
call; ResUNet2.forward_layers decides when it runs.

Arithmetic: the training path never runs on a range-limited one.  Under the process-wide fast mode (ops.CONV_VARIANT 6,
two f16 parts per operand) the forward and the input gradient here run on bf16x3 (variant 3: exact fp32 operands, fp32
range) instead: gradients of the contrastive loss are routinely 1e-5 .. 1e-9, where f16 loses bits (below 6e-5) or
everything (below 6e-8), an activation at or above 65504 would become inf, and this path has neither the range flag nor
the fp32 recompute that guard inference.  Packing costs the same, and the weight gradient is plain fp32 anyway.
tests/test_gpu_backward_exact.py pins it with gradients scaled by 2^-30 and by 2^20.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import ImfError, check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _opposite_rulebook(cm, ts_in, ksize, stride, transposed):
    """Kernel map that carries gradients from the convolution's outputs back to its inputs."""
    if ksize == 1:
        return None
    if not transposed:
        if stride == 1:
            return cm.conv_rulebook(ts_in, ksize, 1)                  # symmetric: same map, flipped offsets
        return cm.transpose_rulebook(ts_in * stride, ksize, stride)  # outputs live at ts_in * stride: coarse -> fine
    return cm.conv_rulebook(ts_in // stride, ksize, stride)          # transposed conv: fine (outputs) -> coarse (inputs)


def training_variant(kvol):
    """The arithmetic of a differentiable convolution: the process-wide one, except that the split-f16 fast mode (6) is
    replaced by bf16x3 (3) -- see the module docstring."""
    variant = ops.conv_variant_for(kvol)
    return 3 if variant == 6 else variant


def conv_flips_taps(module):
    """Whether the input gradient of a sparse convolution runs on the kernel with its taps reversed: stride 1, not
    transposed (the map is its own opposite).  The optimizer's backward images (train/optim.py) follow the same rule."""
    return not module._transposed and module.stride == 1


def spconv_wgrad(feat, grad_out, rb, kvol):
    """dW [kvol, cin, cout] of out = spconv(feat, W, rb)."""
    L = _lib.lib()
    cin, cout = feat.shape[1], grad_out.shape[1]
    dw = torch.empty((kvol, cin, cout), dtype=torch.float32, device=feat.device)
    nbytes = L.imf_spconv_wgrad_workspace_bytes(rb.n_slots, kvol, cin, cout)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=feat.device)
    check(L.imf_spconv_wgrad(feat.data_ptr(), cin, grad_out.data_ptr(), cout,
                             None if rb.tile_rows is None else rb.tile_rows.data_ptr(),
                             None if rb.nbr is None else rb.nbr.data_ptr(), rb.n_slots, rb.n_out, kvol, dw.data_ptr(),
                             ws.data_ptr(), nbytes, _stream()), "imf_spconv_wgrad")
    return dw


class SparseConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, kernel, module, x):
        rb, _ = module.rulebook(x)
        k3 = kernel if kernel.dim() == 3 else kernel.unsqueeze(0)
        feat_c = feat.detach().contiguous()
        if module.in_channels <= 4:
            out = ops.spconv_small_cin(feat_c, k3.detach(), rb)
        else:
            variant = training_variant(module.kernel_volume)
            out = ops.spconv(feat_c, ops.weight_image(kernel, "forward", variant), module.out_channels, rb,
                             variant=variant)
        ctx.save_for_backward(feat_c, kernel)
        ctx.module, ctx.x, ctx.rb = module, x, rb
        return out

    @staticmethod
    def backward(ctx, grad_out):
        feat, kernel = ctx.saved_tensors
        m, x, rb = ctx.module, ctx.x, ctx.rb
        g = grad_out.contiguous().float()
        K = m.kernel_volume
        k3 = kernel.detach() if kernel.dim() == 3 else kernel.detach().unsqueeze(0)
        grad_feat = grad_kernel = None
        if ctx.needs_input_grad[0]:
            if m.in_channels % 32 or m.out_channels % 32:
                raise ImfError("input gradient needs channel counts that are multiples of 32 (the first layer's input "
                               "features do not require grad on IMFNet's path)")
            cm, ts = x.coordinate_manager, x.coordinate_map_key.tensor_stride
            if K == 1:
                grad_feat = g @ k3[0].t()
            else:
                rbt = _opposite_rulebook(cm, ts, m.kernel_size, m.stride, m._transposed)
                variant = training_variant(K)
                wt = ops.weight_image(kernel, "backward", variant, flip=conv_flips_taps(m))
                grad_feat = ops.spconv(g, wt, m.in_channels, rbt, variant=variant)
        if ctx.needs_input_grad[1]:
            dw = spconv_wgrad(feat, g, rb, K)
            grad_kernel = dw if kernel.dim() == 3 else dw[0]
        return grad_feat, grad_kernel, None, None


def _dense_staging(kvol, cout):
    """The launch shape of a dense convolution: the 8-wavefront wave-split kernel imf_image_branch runs its 3x3 layers on,
    the library default (one unsplit k_spconv_g launch) for the pointwise ones.  Static per layer, never a function of the
    batch or image size: the workgroup shape and a split over the taps are part of the summation order."""
    return "wave8" if kvol == 9 and cout % 64 == 0 else None


class DenseConvFunction(torch.autograd.Function):
    """out [rb.n_out, co] = the dense convolution `weight` (torch layout [co, ci, kh, kw], no bias) of the NHWC rows
    `feat` [n_in, ci] over the static pixel table `rb` (ops.ImageTrainTables; kh * kw == rb.kvol).
      d feat    imf_spconv_fwd over `rb_opposite` (rows = the input pixels) with W[k]^T, the taps flipped (k -> K-1-k) when
                `flip` (stride 1: the table is its own opposite); skipped when feat needs no gradient (the stem's im2col)
      d weight  imf_spconv_wgrad over `rb`, permuted back to the parameter's layout."""

    @staticmethod
    def forward(ctx, feat, weight, rb, rb_opposite, flip):
        co, ci, kh, kw = weight.shape
        if kh * kw != rb.kvol or feat.shape[1] != ci:
            raise ImfError(f"DenseConvFunction: weight {tuple(weight.shape)} on a {rb.kvol}-tap table over {feat.shape[1]} channels")
        feat_c = feat.detach().contiguous()
        variant = training_variant(rb.kvol)
        out = ops.spconv(feat_c, ops.weight_image(weight, "forward", variant), co, rb, variant=variant, split_k=1,
                         staging=_dense_staging(rb.kvol, co))
        ctx.save_for_backward(feat_c, weight)
        ctx.rb, ctx.rb_opposite, ctx.flip = rb, rb_opposite, bool(flip)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        feat, weight = ctx.saved_tensors
        rb, rbt = ctx.rb, ctx.rb_opposite
        co, ci, kh, kw = weight.shape
        g = grad_out.contiguous().float()
        grad_feat = grad_weight = None
        if ctx.needs_input_grad[0]:
            if rbt is None or rbt.n_out != feat.shape[0] or rbt.kvol != rb.kvol:
                raise ImfError("DenseConvFunction: the input gradient needs the opposite table of the forward's")
            variant = training_variant(rb.kvol)
            grad_feat = ops.spconv(g, ops.weight_image(weight, "backward", variant, flip=ctx.flip), ci, rbt,
                                   variant=variant, split_k=1, staging=_dense_staging(rb.kvol, ci))
        if ctx.needs_input_grad[1]:
            dw = spconv_wgrad(feat, g, rb, rb.kvol)                          # [k, ci, co]
            grad_weight = dw.view(kh, kw, ci, co).permute(3, 2, 0, 1).contiguous().to(weight.dtype)
        return grad_feat, grad_weight, None, None, None


class MaxPoolRowsFunction(torch.autograd.Function):
    """(out, tap) = nn.MaxPool2d(3, 2, 1) on the NHWC rows x [B*Hin*Win, C] (csrc/image_train.hip): ties go to the first
    maximum in (ky, kx) order as in torch; tap (uint8, not differentiable) is the winner per element.  The backward
    gathers: no atomics."""

    @staticmethod
    def forward(ctx, x, B, Hin, Win):
        out, tap = ops.image_maxpool_forward(x.detach().contiguous(), B, Hin, Win)
        ctx.save_for_backward(tap)
        ctx.shape = (B, Hin, Win)
        ctx.mark_non_differentiable(tap)
        return out, tap

    @staticmethod
    def backward(ctx, grad_out, _grad_tap):
        (tap,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return ops.image_maxpool_backward(grad_out.contiguous().float(), tap, *ctx.shape), None, None, None


class SparseBatchNormFunction(torch.autograd.Function):
    """y = [relu](batch_norm(x) [+ residual]) with batch statistics; `bn` is the nn.BatchNorm1d whose eps, momentum and
    running statistics apply.  The running statistics and num_batches_tracked move exactly when torch moves them:
    training mode with track_running_stats."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, relu):
        track = bn.training and bn.track_running_stats and bn.running_mean is not None
        if track and bn.momentum is None:
            raise ImfError("BatchNorm momentum=None (cumulative moving average) is not implemented by the hip norm "
                           "kernels: use a momentum, or ops.TRAIN_NORM = 'torch'")
        xc = x.detach().contiguous()
        res = None if residual is None else residual.detach().contiguous()
        y, stats = ops.bn_train_forward(xc, gamma.detach().contiguous(), beta.detach().contiguous(), bn.eps, res, relu,
                                        bn.running_mean if track else None, bn.running_var if track else None,
                                        bn.momentum if track else 0.0)
        if track and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        ctx.save_for_backward(xc, y, stats, gamma)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, y, stats, gamma = ctx.saved_tensors
        need_x, need_g, need_b, need_r = ctx.needs_input_grad[:4]
        g = grad_out.contiguous().float()
        if not (need_x or need_g or need_b or need_r):
            return None, None, None, None, None, None
        # without a ReLU the residual's gradient is the incoming gradient itself: no copy
        dx, dgamma, dbeta, dres = ops.bn_train_backward(g, x, y, stats, gamma.detach().contiguous(), ctx.relu, need_x,
                                                        need_g, need_b, need_r and ctx.relu)
        if need_r and not ctx.relu:
            dres = g
        return dx, dgamma, dbeta, dres, None, None


class SparseInstanceNormFunction(torch.autograd.Function):
    """y = [relu](instance_norm(x) [+ residual]) with per-item statistics (csrc/norm_train.hip, imf_in_*).  gamma / beta
    are the module's [1, C] parameters; item_starts is the int32 [n_items + 1] device array of the rows' partition."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, item_starts, relu):
        from .sparse import MinkowskiInstanceNorm
        xc = x.detach().contiguous()
        res = None if residual is None else residual.detach().contiguous()
        y, stats = ops.in_forward(xc, item_starts, gamma.detach().reshape(-1).contiguous(),
                                  beta.detach().reshape(-1).contiguous(), MinkowskiInstanceNorm.EPS, res, relu)
        ctx.save_for_backward(xc, y, stats, gamma, item_starts)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, y, stats, gamma, item_starts = ctx.saved_tensors
        need_x, need_g, need_b, need_r = ctx.needs_input_grad[:4]
        g = grad_out.contiguous().float()
        if not (need_x or need_g or need_b or need_r):
            return None, None, None, None, None, None
        # without a ReLU the residual's gradient is the incoming gradient itself: no copy
        dx, dgamma, dbeta, dres = ops.in_backward(g, x, y, stats, gamma.detach().reshape(-1).contiguous(), item_starts,
                                                  ctx.relu, need_x, need_g, need_b, need_r and ctx.relu)
        if need_r and not ctx.relu:
            dres = g
        return (dx, None if dgamma is None else dgamma.view_as(gamma), None if dbeta is None else dbeta.view_as(gamma),
                dres, None, None)


class HardestContrastiveLossFunction(torch.autograd.Function):
    """(pos_loss, neg_loss, hard01, hard10) of csrc/loss.hip (ops.TRAIN_LOSS == "hip"): the two losses as 0-d device
    tensors, the hardest negatives as global rows (int64, not differentiable).  pairs / pos_sel / sel0 / sel1 are int64
    device tensors (pos_sel None: every pair).  The backward hands the two incoming gradients to the kernels as one
    2-element device tensor; nothing on either way waits for the device."""

    @staticmethod
    def forward(ctx, F0, F1, pairs, pos_sel, sel0, sel1, pos_thresh, neg_thresh):
        f0, f1 = F0.detach().float().contiguous(), F1.detach().float().contiguous()
        loss, hard01, hard10, keep01, keep10, meta = ops.hc_loss_forward(f0, f1, pairs, pos_sel, sel0, sel1, pos_thresh,
                                                                         neg_thresh)
        ctx.save_for_backward(f0, f1, pairs, pos_sel, sel0, sel1, hard01, hard10, keep01, keep10, meta)
        ctx.thresh = (float(pos_thresh), float(neg_thresh))
        ctx.dtypes = (F0.dtype, F1.dtype)
        ctx.mark_non_differentiable(hard01, hard10)
        return loss[0], loss[1], hard01, hard10

    @staticmethod
    def backward(ctx, grad_pos, grad_neg, _g01, _g10):
        f0, f1, pairs, pos_sel, sel0, sel1, hard01, hard10, keep01, keep10, meta = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 8
        zero = f0.new_zeros(())
        grad = torch.stack([zero if grad_pos is None else grad_pos.float().reshape(()),
                            zero if grad_neg is None else grad_neg.float().reshape(())]).contiguous()
        df0, df1 = ops.hc_loss_backward(f0, f1, pairs, pos_sel, sel0, sel1, *ctx.thresh, hard01, hard10, keep01, keep10,
                                        meta, grad)
        return (df0.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None,
                df1.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None)


class AttentionFusionFunction(torch.autograd.Function):
    """z = AttentionFusion(tokens, queries_encoder=x) of model/fusion.py (depth 0, one head) for every batch item at
    once: x [n, 256] rows grouped by item, item_starts int32 [items + 1] on the device (ops.fusion_item_starts), tokens
    [items, T, 128], then the block's 14 parameters in the order of ops.FUSION_TRAIN_PARAMS.  The backward computes only
    the gradients autograd asks for; nothing on either way waits for the device."""

    @staticmethod
    def forward(ctx, x, item_starts, tokens, *params):
        xc, tc = x.detach().contiguous(), tokens.detach().contiguous()
        weights = [p.detach().contiguous() for p in params]
        z, saved, _meta = ops.fusion_train_forward(xc, item_starts, tc, weights)
        ctx.save_for_backward(xc, item_starts, tc, saved, *weights)
        return z

    @staticmethod
    def backward(ctx, grad_out):
        xc, item_starts, tc, saved, *weights = ctx.saved_tensors
        need = ctx.needs_input_grad
        none = (None,) * (3 + len(weights))
        if not any(need):
            return none
        if xc.shape[0] == 0:                         # no rows: the kernels launch nothing, every gradient is zero
            return tuple(torch.zeros_like(t) if k else None for t, k in zip((xc, item_starts, tc, *weights), need))
        dx, dtok, grads, _meta = ops.fusion_train_backward(grad_out.contiguous().float(), xc, item_starts, tc, weights,
                                                           saved, need[0], need[2], need[3:])
        return (dx, None, dtok, *grads)


class HeadFunction(torch.autograd.Function):
    """y = the descriptor head of forward_layers on feature rows (csrc/head_train.hip, ops.TRAIN_HEAD == "hip"):
    relu(cat(u, s) @ w1) @ w2 + bias, divided by its rows' L2 norms when `normalize`.  u [n, 64], s [n, 32], w1 [96, 64]
    (conv1_tr.kernel), w2 [64, 32] and bias [1, 32] (final).  Saves u, s, h, r, y; the backward computes only the gradients
    autograd asks for; nothing on either way waits for the device."""

    @staticmethod
    def forward(ctx, u, s, w1, w2, bias, normalize):
        uc, sc = u.detach().contiguous(), s.detach().contiguous()
        w1c, w2c, bc = w1.detach().contiguous(), w2.detach().contiguous(), bias.detach().contiguous()
        h, r, y, _meta = ops.head_train_forward(uc, sc, w1c, w2c, bc, normalize)
        ctx.normalize = bool(normalize)
        ctx.save_for_backward(uc, sc, h, r, y, w1c, w2c)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        u, s, h, r, y, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad[:5]
        if not any(need):
            return (None,) * 6
        du, ds, dw1, dw2, db, _meta = ops.head_train_backward(grad_out.contiguous().float(), y, r, h, u, s, w1, w2,
                                                             ctx.normalize, want=need)
        return du, ds, dw1, dw2, db, None
