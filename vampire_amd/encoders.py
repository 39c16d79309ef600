"""Build-owned image / BEV encoders standing where the reference calls mmdet's `build_backbone` and
mmdet3d's `build_neck` (base_vampire2.py:167-168, bev_depth_head.py:131-134): ResNet-18/34/50 and the
SECOND FPN, with mmdet's constructor arguments and attribute names and torchvision's parameter
names (so `torchvision://resnet50` state dicts load).  mmdet / mmdet3d are not in this image; these
are implementations of the published architectures, not copies -- "parity unpinned" against the
registry versions."""
import torch
import torch.nn.functional as F
from torch import nn

from .norm import build_norm, is_fused


# =============================================================================================
class _BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, planes, stride=1, downsample=None, norm_cfg=None):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 3, stride, 1, bias=False)
        self.bn1 = build_norm(norm_cfg, planes, act="relu")
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = build_norm(norm_cfg, planes, act="relu")
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        if is_fused(self.bn1):                                 # SyncBN: the norms carry the ReLUs and the residual
            return self.bn2(self.conv2(self.bn1(self.conv1(x))), idt)
        y = F.relu(self.bn1(self.conv1(x)), inplace=True)
        return F.relu(self.bn2(self.conv2(y)) + idt, inplace=True)


class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin, planes, stride=1, downsample=None, norm_cfg=None):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = build_norm(norm_cfg, planes, act="relu")
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)       # style='pytorch': stride on the 3x3
        self.bn2 = build_norm(norm_cfg, planes, act="relu")
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = build_norm(norm_cfg, planes * 4, act="relu")
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        if is_fused(self.bn1):
            return self.bn3(self.conv3(self.bn2(self.conv2(self.bn1(self.conv1(x))))), idt)
        y = F.relu(self.bn1(self.conv1(x)), inplace=True)
        y = F.relu(self.bn2(self.conv2(y)), inplace=True)
        return F.relu(self.bn3(self.conv3(y)) + idt, inplace=True)


class ResNet(nn.Module):
    """ResNet-18/34/50 trunk with mmdet's constructor arguments and attribute names (`conv1 norm1 relu
    maxpool res_layers out_indices deep_stem`, layers `layer1..`), torchvision parameter names."""
    ARCH = {18: (_BasicBlock, (2, 2, 2, 2)), 34: (_BasicBlock, (3, 4, 6, 3)), 50: (_Bottleneck, (3, 4, 6, 3))}

    def __init__(self, depth=50, in_channels=3, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), norm_eval=False, frozen_stages=-1,
                 init_cfg=None, type=None, norm_cfg=None, **_):
        super().__init__()
        block, blocks = self.ARCH[depth]
        self.deep_stem = False
        self.out_indices = list(out_indices)
        self.conv1 = nn.Conv2d(in_channels, base_channels, 7, 2, 3, bias=False)
        self.bn1 = build_norm(norm_cfg, base_channels, act="relu")
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.res_layers = []
        cin = base_channels
        for i in range(num_stages):
            planes = base_channels * 2 ** i
            layers = []
            for j in range(blocks[i]):
                stride = strides[i] if j == 0 else 1
                down = None
                if stride != 1 or cin != planes * block.expansion:
                    down = nn.Sequential(nn.Conv2d(cin, planes * block.expansion, 1, stride, bias=False),
                                         build_norm(norm_cfg, planes * block.expansion))
                layers.append(block(cin, planes, stride, down, norm_cfg))
                cin = planes * block.expansion
            name = f"layer{i + 1}"
            setattr(self, name, nn.Sequential(*layers))
            self.res_layers.append(name)

    @property
    def norm1(self):
        return self.bn1

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def stem(self, x):
        """conv1 + norm1 + ReLU (one node with a fused norm)."""
        x = self.bn1(self.conv1(x))
        return x if is_fused(self.bn1) else self.relu(x)

    def forward(self, x):
        x = self.stem(x)
        if hasattr(self, "maxpool"):
            x = self.maxpool(x)
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return outs


class SECONDFPN(nn.Module):
    """Every level resampled to one stride (transposed conv up, strided conv down), BN + ReLU, concat."""

    def __init__(self, in_channels, out_channels, upsample_strides, type=None, norm_cfg=None, **_):
        super().__init__()
        norm_cfg = dict(dict(type="BN", eps=1e-3, momentum=0.01), **(norm_cfg or {}))
        blocks = []
        for cin, cout, s in zip(in_channels, out_channels, upsample_strides):
            if s >= 1:
                s = int(round(s))
                layer = nn.ConvTranspose2d(cin, cout, s, s, bias=False)
            else:
                k = int(round(1.0 / s))
                layer = nn.Conv2d(cin, cout, k, k, bias=False)
            norm = build_norm(norm_cfg, cout, act="relu")
            blocks.append(nn.Sequential(layer, norm, nn.Identity() if is_fused(norm) else nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(blocks)

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, xs):
        return [torch.cat([blk(x) for blk, x in zip(self.deblocks, xs)], dim=1)]


def build_backbone(conf):
    return ResNet(**conf)


def build_neck(conf):
    return SECONDFPN(**conf)


