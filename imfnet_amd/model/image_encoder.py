"""Image branch: ResNet-34 trunk truncated after layer2.

Interface parity with the reference (model/Img_Encoder.py:9-18, model/resnet.py:118-224):
`ImageEncoder().backbone` is a torchvision-layout ResNet-34 (parameter names conv1, bn1,
layer{1..4}.{i}.conv{1,2} / bn{1,2} / downsample.{0,1}, fc), so reference checkpoints -- which store
all 218 backbone tensors although only conv1..layer2 are ever executed (resnet.py:205-216) -- load
with strict=True.  `forward` returns the stride-8 map [B,128,H/8,W/8].

Unlike the reference, construction never touches the network (resnet.py:222 downloads ImageNet
weights that the checkpoint then overwrites).

Training (ops.TRAIN_IMAGE == "hip", python -m imfnet_amd.train --image_kernels hip): `ImageEncoder.forward` runs the
executed part of the trunk on NHWC rows through the library's deterministic kernels (`_forward_kernels`); with the
switch off, in eval mode, without autograd, on the CPU or on another backbone the torch modules run as they always did.
"""
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))


class ResNet(nn.Module):
    """torchvision ResNet skeleton; `forward` stops after layer2 (reference resnet.py:195-216)."""

    def __init__(self, in_channels=3, layers=(3, 4, 6, 3), num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._stage(64, layers[0], 1)
        self.layer2 = self._stage(128, layers[1], 2)
        self.layer3 = self._stage(256, layers[2], 2)      # stored in checkpoints, never executed
        self.layer4 = self._stage(512, layers[3], 2)      # "
        self.fc = nn.Linear(512, num_classes)             # "
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    def _stage(self, planes, blocks, stride):
        down = None
        if stride != 1 or self.inplanes != planes:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes, 1, stride, bias=False),
                                 nn.BatchNorm2d(planes))
        mods = [BasicBlock(self.inplanes, planes, stride, down)]
        self.inplanes = planes
        mods += [BasicBlock(planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*mods)

    def forward(self, x):
        x = self.maxpool(F.relu(self.bn1(self.conv1(x))))
        return self.layer2(self.layer1(x))


def resnet34(in_channels=3, pretrained=False, progress=True, **kwargs):
    """`pretrained` is accepted for signature parity and ignored: weights come from the IMFNet
    checkpoint's state_dict (scripts/generate_desc.py:174)."""
    return ResNet(in_channels, (3, 4, 6, 3), **kwargs)


def trunk_supported(bb):
    """Whether `bb` is the trunk the library's image kernels implement (csrc/image.hip, csrc/image_train.hip): the 7x7
    stem on 3 channels, three plain blocks in layer1, four in layer2 of which only the first projects its identity, on
    the GPU.  ImagePlan (inference) and ImageEncoder's training path both ask this."""
    return (len(bb.layer1) == 3 and len(bb.layer2) == 4 and bb.conv1.weight.is_cuda and
            bb.conv1.weight.shape == (64, 3, 7, 7) and bb.layer2[0].downsample is not None and
            all(b.downsample is None for b in list(bb.layer1) + list(bb.layer2)[1:]))


class ImageEncoder(nn.Module):
    MAX_TRAIN_TABLES = 4                   # image shapes whose pixel tables stay cached (least recently used goes)

    def __init__(self):
        super().__init__()
        self.backbone = resnet34(in_channels=3, pretrained=False)
        self._train_tables = OrderedDict()  # (device, B, H, W) -> ops.ImageTrainTables; no part of the state_dict

    def __getstate__(self):
        """copy.deepcopy and pickling (torch.save of the module) leave the cached tables behind: they are rebuilt from
        (B, H, W) on first use."""
        state = dict(self.__dict__)
        state["_train_tables"] = OrderedDict()
        return state

    def executed_norms(self):
        """The 16 BatchNorm2d modules `forward` runs, in execution order (layer2.0: bn1, downsample, bn2)."""
        bb = self.backbone
        norms = [bb.bn1]
        for blk in list(bb.layer1) + list(bb.layer2):
            norms.append(blk.bn1)
            if blk.downsample is not None:
                norms.append(blk.downsample[1])
            norms.append(blk.bn2)
        return norms

    def executed_convs(self):
        """(convolution, flip) of the 15 convolutions `_forward_kernels` hands to DenseConvFunction with their own weight
        (not the stem: its matrix is a derived tensor), `flip` as it passes it: the stride-1 ones run their input gradient
        on the flipped taps.  train.optim.FusedSGD keeps the weight images of exactly these."""
        bb = self.backbone
        out = []
        for blk in list(bb.layer1) + list(bb.layer2):
            strided = blk.downsample is not None
            out.append((blk.conv1, not strided))
            out.append((blk.conv2, True))
            if strided:
                out.append((blk.downsample[0], False))
        return out

    def _kernels_apply(self, x):
        """Whether this call takes the kernel path: the switch, training mode under autograd, an fp32 GPU image that
        needs no gradient, the backbone model/image_plan.py's ImagePlan supports, two rows or more at every stage."""
        from .. import ops
        if ops.TRAIN_IMAGE != "hip" or not self.training or not torch.is_grad_enabled():
            return False
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and
                not x.requires_grad and x.shape[2] >= 8 and x.shape[3] >= 8):
            return False
        bb = self.backbone
        if not (trunk_supported(bb) and bb.conv1.weight.dtype == torch.float32):
            return False
        # momentum=None (cumulative average) is not implemented by the norm kernels: such a module runs the torch body
        if not all(isinstance(n, nn.BatchNorm2d) and n.training and n.affine and n.momentum is not None
                   for n in self.executed_norms()):
            return False
        _, _, (h8, w8) = ops.image_trunk_shapes(x.shape[2], x.shape[3])
        return x.shape[0] * h8 * w8 >= 2

    def _forward_kernels(self, x, trace=None):
        """conv7x7/2 - bn - relu - maxpool - layer1 - layer2 on NHWC rows [B*H*W, C] (csrc/image_train.hip, autograd.py):
        im2col + a pointwise convolution for the stem, one DenseConvFunction per convolution over the static pixel
        tables, SparseBatchNormFunction (BatchNorm2d over NCHW is BatchNorm over the rows) with the block's ReLU and
        residual add folded in.  `trace` (a list) receives every ReLU output and the pool's tap tensor in execution order."""
        from .. import ops
        from ..autograd import DenseConvFunction, MaxPoolRowsFunction, SparseBatchNormFunction
        bb = self.backbone
        B, _, H, W = x.shape
        key = (x.device, B, H, W)
        tabs = self._train_tables.get(key)
        if tabs is None:
            tabs = self._train_tables[key] = ops.ImageTrainTables(B, H, W, x.device)
            while len(self._train_tables) > self.MAX_TRAIN_TABLES:
                self._train_tables.popitem(last=False)
        else:
            self._train_tables.move_to_end(key)
        (h2, w2), _, (h8, w8) = tabs.shapes

        def norm(rows, bn, residual, relu):
            y = SparseBatchNormFunction.apply(rows, bn.weight, bn.bias, residual, bn, relu)
            if relu and trace is not None:
                trace.append(y)
            return y

        # stem: the [64,3,7,7] weight as the [160, 64] matrix of the im2col columns (ky*7+kx)*3 + ch, rows 147..159 zero
        w = bb.conv1.weight.permute(2, 3, 1, 0).reshape(147, 64)
        w = torch.cat([w, w.new_zeros((13, 64))]).t().reshape(64, 160, 1, 1)
        y = DenseConvFunction.apply(ops.image_im2col7(x.contiguous()), w, tabs.stem, None, False)
        y = norm(y, bb.bn1, None, True)
        y, tap = MaxPoolRowsFunction.apply(y, B, h2, w2)
        if trace is not None:
            trace.append(tap)
        for blk in list(bb.layer1) + list(bb.layer2):
            strided = blk.downsample is not None
            t_in, t_out = (tabs.t4 if blk.conv1.in_channels == 64 else tabs.t8), (tabs.t4 if blk.conv2.out_channels == 64 else tabs.t8)
            if strided:
                z = DenseConvFunction.apply(y, blk.conv1.weight, tabs.t48, tabs.t48T, False)
            else:
                z = DenseConvFunction.apply(y, blk.conv1.weight, t_in, t_in, True)
            z = norm(z, blk.bn1, None, True)
            z = DenseConvFunction.apply(z, blk.conv2.weight, t_out, t_out, True)
            if strided:
                y = norm(DenseConvFunction.apply(y, blk.downsample[0].weight, tabs.td, tabs.tdT, False), blk.downsample[1],
                         None, False)
            y = norm(z, blk.bn2, y, True)
        return y.view(B, h8, w8, y.shape[1]).permute(0, 3, 1, 2)

    def forward(self, x, trace=None):
        if self._kernels_apply(x):
            return self._forward_kernels(x, trace)
        return self.backbone(x)
