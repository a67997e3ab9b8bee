"""FCN-32s (ResNet-101-v1c backbone): model/fcn/voc.fcn32s.R101_v1c/network.py:13-71 on the furnace surface.

Attribute names and construction order follow the reference file (FCN :13-47, _FCNHead :50-66), so state dicts are
interchangeable and a fixed seed initialises both identically (tests/test_fcn_cpu.py).  The backbone is NOT dilated:
the heads read the 1/32 (layer4) and 1/16 (layer3) maps and up-sample them by 32 and 16 into
nn.CrossEntropyLoss(ignore_index=255); on HIP tensors those up-samplings stay deferred into the fused criterion
(upsample_logits / head_loss).  Without a label the forward returns the raw up-sampled logits, as the reference does
(no log_softmax: the Evaluator's exp() of them is what the reference scores).
"""
import torch.nn as nn
import torch.nn.functional as F

from . import ensure_furnace_on_path, head_loss, upsample_logits

ensure_furnace_on_path()
from base_model import resnet101  # noqa: E402
from seg_opr.seg_oprs import ConvBnRelu  # noqa: E402

AUX_LOSS_RATIO = 0.5            # voc.fcn32s.R101_v1c config.py:84


class FCN(nn.Module):
    tsg_native_fusions = True      # calls the fused operators itself (workloads/__init__.py)

    def __init__(self, out_planes, criterion, inplace=True, pretrained_model=None, norm_layer=nn.BatchNorm2d,
                 bn_eps=1e-5, bn_momentum=0.1, aux_loss_ratio=AUX_LOSS_RATIO):
        super(FCN, self).__init__()
        self.backbone = resnet101(pretrained_model, inplace=inplace, norm_layer=norm_layer, bn_eps=bn_eps,
                                  bn_momentum=bn_momentum, deep_stem=True, stem_width=64)
        self.business_layer = []
        self.head = _FCNHead(2048, out_planes, inplace, norm_layer=norm_layer)
        self.aux_head = _FCNHead(1024, out_planes, inplace, norm_layer=norm_layer)
        self.business_layer.append(self.head)
        self.business_layer.append(self.aux_head)
        self.criterion = criterion
        self.aux_loss_ratio = aux_loss_ratio

    def forward(self, data, label=None):
        blocks = self.backbone(data)
        fm = self.head(blocks[-1])
        if label is not None:                                                     # network.py:39-44
            pred = upsample_logits(fm, scale=32)
            aux_pred = upsample_logits(self.aux_head(blocks[-2]), scale=16)
            return head_loss(self.criterion, pred, label) + self.aux_loss_ratio * head_loss(self.criterion, aux_pred,
                                                                                              label)
        # evaluation: the literal statement (FuseMode(infer=True) of torchseg_amd.infer keeps it pending when it is active)
        return F.interpolate(fm, scale_factor=32, mode='bilinear', align_corners=True)


class _FCNHead(nn.Module):
    def __init__(self, in_planes, out_planes, inplace=True, norm_layer=nn.BatchNorm2d):
        super(_FCNHead, self).__init__()
        inter_planes = in_planes // 4
        self.cbr = ConvBnRelu(in_planes, inter_planes, 3, 1, 1, has_bn=True, norm_layer=norm_layer, has_relu=True,
                              inplace=inplace, has_bias=False)
        self.dropout = nn.Dropout2d(0.1)
        self.conv1x1 = nn.Conv2d(inter_planes, out_planes, kernel_size=1, stride=1, padding=0)

    def forward(self, x):
        return self.conv1x1(self.dropout(self.cbr(x)))
