"""Xception39, the context path of BiSeNet-X39 (model/bisenet/cityscapes.bisenet.X39/network.py:10,22), with the surface
of the reference's furnace/base_model/xception.py: `xception39(pretrained_model=None, norm_layer=)`, forward returns the
three stage outputs (1/8, 1/16, 1/32), attribute names and construction order unchanged so that state dicts interchange
and a fixed seed initialises both identically (tests/test_bisenet_x39_cpu.py).

The backbone's separable convolution is a depthwise 3x3 convolution straight into the point-wise ConvBnRelu — no
BatchNorm in between, unlike seg_oprs.SeparableConvBnRelu.  Its 51 depthwise layers run on our kernels once the DDP
wrapper has installed torchseg_amd.dwconv.  With torchseg_amd's SyncBatchNorm the last point-wise BatchNorm of a block,
the shortcut addition and the ReLU are one normalise kernel (norm_act with a residual).
"""
import torch
import torch.nn as nn

from seg_opr.seg_oprs import ConvBnRelu, norm_act
from torchseg_amd.pool import MaxPool2d as _MaxPool2d
from utils.pyt_utils import load_model

__all__ = ['Xception', 'xception39']


class SeparableConvBnRelu(nn.Module):
    """depthwise k x k convolution -> point-wise ConvBnRelu"""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, dilation=1,
                 has_relu=True, norm_layer=nn.BatchNorm2d):
        super(SeparableConvBnRelu, self).__init__()
        self.conv1 = nn.Conv2d(in_channels, in_channels, kernel_size, stride, padding, dilation,
                               groups=in_channels, bias=False)
        self.point_wise_cbr = ConvBnRelu(in_channels, out_channels, 1, 1, 0, has_bn=True, norm_layer=norm_layer,
                                         has_relu=has_relu, has_bias=False)

    def forward(self, x):
        return self.point_wise_cbr(self.conv1(x))

    def forward_residual(self, x, residual, relu):
        """relu(bn(point-wise conv(depthwise conv(x))) + residual) with the BatchNorm, the addition and the ReLU fused"""
        pw = self.point_wise_cbr
        return norm_act(pw.bn, relu, pw.conv(self.conv1(x)), residual=residual)


class Block(nn.Module):
    expansion = 4

    def __init__(self, in_channels, mid_out_channels, has_proj, stride, dilation=1, norm_layer=nn.BatchNorm2d):
        super(Block, self).__init__()
        self.has_proj = has_proj
        out_channels = mid_out_channels * self.expansion
        if has_proj:
            self.proj = SeparableConvBnRelu(in_channels, out_channels, 3, stride, 1, has_relu=False,
                                            norm_layer=norm_layer)
        self.residual_branch = nn.Sequential(
            SeparableConvBnRelu(in_channels, mid_out_channels, 3, stride, dilation, dilation, has_relu=True,
                                norm_layer=norm_layer),
            SeparableConvBnRelu(mid_out_channels, mid_out_channels, 3, 1, 1, has_relu=True, norm_layer=norm_layer),
            SeparableConvBnRelu(mid_out_channels, out_channels, 3, 1, 1, has_relu=False, norm_layer=norm_layer))
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        shortcut = self.proj(x) if self.has_proj else x
        r = self.residual_branch[1](self.residual_branch[0](x))
        return self.residual_branch[2].forward_residual(r, shortcut, self.relu)


class Xception(nn.Module):
    def __init__(self, block, layers, channels, norm_layer=nn.BatchNorm2d):
        super(Xception, self).__init__()
        self.in_channels = 8
        self.conv1 = ConvBnRelu(3, self.in_channels, 3, 2, 1, has_bn=True, norm_layer=norm_layer, has_relu=True,
                                has_bias=False)
        self.maxpool = _MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, norm_layer, layers[0], channels[0], stride=2)
        self.layer2 = self._make_layer(block, norm_layer, layers[1], channels[1], stride=2)
        self.layer3 = self._make_layer(block, norm_layer, layers[2], channels[2], stride=2)

    def _make_layer(self, block, norm_layer, blocks, mid_out_channels, stride=1):
        stages = [block(self.in_channels, mid_out_channels, stride > 1, stride=stride, norm_layer=norm_layer)]
        self.in_channels = mid_out_channels * block.expansion
        for _ in range(1, blocks):
            stages.append(block(self.in_channels, mid_out_channels, has_proj=False, stride=1, norm_layer=norm_layer))
        return nn.Sequential(*stages)

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        if x.is_cuda:
            # the 3 -> 8 stem stays on the vendor library, whose output follows the image's NCHW layout; the depthwise
            # kernels (torchseg_amd.dwconv) take channels_last maps: one copy of the pooled 1/4 map here
            x = x.contiguous(memory_format=torch.channels_last)
        blocks = []
        for layer in (self.layer1, self.layer2, self.layer3):
            x = layer(x)
            blocks.append(x)
        return blocks


def xception39(pretrained_model=None, **kwargs):
    model = Xception(Block, [4, 8, 4], [16, 32, 64], **kwargs)
    if pretrained_model is not None:
        model = load_model(model, pretrained_model)
    return model
