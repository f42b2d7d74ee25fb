"""Plain-PyTorch definitions of the reference's model families (test oracle).

The reference loads ``torch.hub.load('pytorch/vision:v0.10.0', 'alexnet' |
'resnet18', pretrained=True)`` on every chunk (reference alexnet_resnet.py:17-22).
torchvision is not part of this framework; these modules re-state the same
architectures (torchvision v0.10 layer lists: SURVEY.md §2.4) with the same
``state_dict`` key names, so real pretrained weights saved as safetensors load
unchanged.  They are used

  * as the numerics oracle for the HIP kernels (fp32, CPU or GPU), and
  * as the CPU executor of the cluster when no GPU is present.

Random init follows torchvision's: kaiming-normal(fan_out) convs, BN
gamma=1/beta=0, running stats (0, 1); Linear default init.
"""
from __future__ import annotations

import threading

import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv(cin, cout, k, s=1, p=0, groups=1):
    return nn.Conv2d(cin, cout, k, stride=s, padding=p, groups=groups, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, width, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        self.conv1 = _conv(cin, width, 3, stride, 1)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv(width, width, 3, 1, 1)
        self.bn2 = nn.BatchNorm2d(width)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + idt)


class Bottleneck(nn.Module):
    """ResNet v1.5 bottleneck: the stride sits on the 3x3 conv.  ``groups`` and
    ``base_width`` are torchvision's: the inner width is
    ``int(planes * base_width / 64) * groups`` (ResNeXt: 32 groups of 4 or 8
    channels per 64 planes; Wide ResNet: base_width 128), conv2 is grouped, and
    the block's output stays ``planes * 4``."""

    expansion = 4

    def __init__(self, cin, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = int(planes * base_width / 64) * groups
        self.conv1 = _conv(cin, width, 1)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv(width, width, 3, stride, 1, groups)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = _conv(width, planes * 4, 1)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return F.relu(y + idt)


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000, groups=1, width_per_group=64):
        super().__init__()
        self.groups, self.base_width = groups, width_per_group
        self.conv1 = _conv(3, 64, 7, 2, 3)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for i, (n, width) in enumerate(zip(layers, (64, 128, 256, 512))):
            stride = 1 if i == 0 else 2
            blocks = []
            for j in range(n):
                s = stride if j == 0 else 1
                ds = None
                if j == 0 and (s != 1 or cin != width * block.expansion):
                    ds = nn.Sequential(_conv(cin, width * block.expansion, 1, s),
                                       nn.BatchNorm2d(width * block.expansion))
                blocks.append(block(cin, width, s, ds, groups, width_per_group))
                cin = width * block.expansion
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.maxpool(F.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class AlexNet(nn.Module):
    def __init__(self, num_classes=1000):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
        )
        self.avgpool = nn.AdaptiveAvgPool2d((6, 6))
        self.classifier = nn.Sequential(
            nn.Dropout(), nn.Linear(256 * 36, 4096), nn.ReLU(inplace=True),
            nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(inplace=True),
            nn.Linear(4096, num_classes),
        )

    def forward(self, x):
        x = self.avgpool(self.features(x))
        return self.classifier(torch.flatten(x, 1))


def _conv_bn_relu6(cin, cout, k=3, s=1, groups=1):
    """torchvision v0.10's ConvBNActivation: [Conv2d(bias=False), BatchNorm2d, ReLU6]."""
    return nn.Sequential(_conv(cin, cout, k, s, (k - 1) // 2, groups), nn.BatchNorm2d(cout), nn.ReLU6(inplace=True))


class InvertedResidual(nn.Module):
    """MobileNetV2 block: [1x1 expand-BN-ReLU6 (absent at t = 1)], depthwise
    3x3-BN-ReLU6, 1x1 project, BN; + x where stride 1 and cin == cout, and no
    activation after the add."""

    def __init__(self, cin, cout, stride, t):
        super().__init__()
        hidden = cin * t
        self.use_res = stride == 1 and cin == cout
        layers = [_conv_bn_relu6(cin, hidden, 1)] if t != 1 else []
        layers += [_conv_bn_relu6(hidden, hidden, 3, stride, groups=hidden), _conv(hidden, cout, 1),
                   nn.BatchNorm2d(cout)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res else self.conv(x)


MOBILENET_V2_SETTINGS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2),
                         (6, 320, 1, 1))       # (t, c, n, s)


class MobileNetV2(nn.Module):
    """torchvision v0.10's mobilenet_v2 at width 1.0 (3,504,872 parameters)."""

    def __init__(self, num_classes=1000):
        super().__init__()
        feats, cin = [_conv_bn_relu6(3, 32, 3, 2)], 32
        for t, c, n, s in MOBILENET_V2_SETTINGS:
            for i in range(n):
                feats.append(InvertedResidual(cin, c, s if i == 0 else 1, t))
                cin = c
        feats.append(_conv_bn_relu6(cin, 1280, 1))
        self.features = nn.Sequential(*feats)
        self.classifier = nn.Sequential(nn.Dropout(0.2), nn.Linear(1280, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.features(x).mean(dim=(2, 3))
        return self.classifier(x)


def mobilenet_v2(num_classes=1000):
    return MobileNetV2(num_classes)


def _make_divisible(v, divisor=8):
    """torchvision's channel rounding: to the nearest multiple of ``divisor``, never below 90 % of ``v``."""
    n = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return n + divisor if n < 0.9 * v else n


def _conv_bn_act(cin, cout, k, s, groups, act):
    """torchvision v0.10's ConvBNActivation as MobileNetV3 builds it: BN eps 0.001, momentum 0.01;
    ``act`` is an activation class or None."""
    layers = [_conv(cin, cout, k, s, (k - 1) // 2, groups), nn.BatchNorm2d(cout, eps=0.001, momentum=0.01)]
    return nn.Sequential(*layers, *([act(inplace=True)] if act is not None else []))


class SqueezeExcitation(nn.Module):
    """torchvision v0.10's: x * hardsigmoid(fc2(relu(fc1(mean_hw(x))))), both FCs 1x1 convs with bias."""

    def __init__(self, channels, squeeze_factor=4):
        super().__init__()
        squeeze = _make_divisible(channels // squeeze_factor, 8)
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)

    def forward(self, x):
        scale = F.relu(self.fc1(x.mean(dim=(2, 3), keepdim=True)))
        return F.hardsigmoid(self.fc2(scale)) * x


class InvertedResidualV3(nn.Module):
    """MobileNetV3 block: [1x1 expand-BN-act (absent when expanded == cin)], depthwise
    k x k-BN-act, [SE], 1x1 project-BN; + x where stride 1 and cin == cout."""

    def __init__(self, cin, k, expanded, cout, se, hs, stride):
        super().__init__()
        act = nn.Hardswish if hs else nn.ReLU
        self.use_res = stride == 1 and cin == cout
        layers = [_conv_bn_act(cin, expanded, 1, 1, 1, act)] if expanded != cin else []
        layers.append(_conv_bn_act(expanded, expanded, k, stride, expanded, act))
        if se:
            layers.append(SqueezeExcitation(expanded))
        layers.append(_conv_bn_act(expanded, cout, 1, 1, 1, None))
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.block(x) if self.use_res else self.block(x)


# (cin, kernel, expanded, cout, SE, hardswish (else ReLU), stride)
MOBILENET_V3_SETTINGS = {
    "large": ((16, 3, 16, 16, False, False, 1), (16, 3, 64, 24, False, False, 2), (24, 3, 72, 24, False, False, 1),
              (24, 5, 72, 40, True, False, 2), (40, 5, 120, 40, True, False, 1), (40, 5, 120, 40, True, False, 1),
              (40, 3, 240, 80, False, True, 2), (80, 3, 200, 80, False, True, 1), (80, 3, 184, 80, False, True, 1),
              (80, 3, 184, 80, False, True, 1), (80, 3, 480, 112, True, True, 1), (112, 3, 672, 112, True, True, 1),
              (112, 5, 672, 160, True, True, 2), (160, 5, 960, 160, True, True, 1), (160, 5, 960, 160, True, True, 1)),
    "small": ((16, 3, 16, 16, True, False, 2), (16, 3, 72, 24, False, False, 2), (24, 3, 88, 24, False, False, 1),
              (24, 5, 96, 40, True, True, 2), (40, 5, 240, 40, True, True, 1), (40, 5, 240, 40, True, True, 1),
              (40, 5, 120, 48, True, True, 1), (48, 5, 144, 48, True, True, 1), (48, 5, 288, 96, True, True, 2),
              (96, 5, 576, 96, True, True, 1), (96, 5, 576, 96, True, True, 1)),
}
MOBILENET_V3_LAST_CHANNEL = {"large": 1280, "small": 1024}


class MobileNetV3(nn.Module):
    """torchvision v0.10's mobilenet_v3_large (5,483,032 parameters) / mobilenet_v3_small
    (2,542,856) at width 1.0."""

    def __init__(self, arch, num_classes=1000):
        super().__init__()
        self.arch = arch
        settings = MOBILENET_V3_SETTINGS[arch]
        feats = [_conv_bn_act(3, settings[0][0], 3, 2, 1, nn.Hardswish)]
        feats += [InvertedResidualV3(*row) for row in settings]
        cin = settings[-1][3]
        feats.append(_conv_bn_act(cin, 6 * cin, 1, 1, 1, nn.Hardswish))
        self.features = nn.Sequential(*feats)
        last = MOBILENET_V3_LAST_CHANNEL[arch]
        self.classifier = nn.Sequential(nn.Linear(6 * cin, last), nn.Hardswish(inplace=True),
                                        nn.Dropout(0.2, inplace=True), nn.Linear(last, num_classes))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.features(x).mean(dim=(2, 3))
        return self.classifier(x)


def mobilenet_v3_large(num_classes=1000):
    return MobileNetV3("large", num_classes)


def mobilenet_v3_small(num_classes=1000):
    return MobileNetV3("small", num_classes)


class Fire(nn.Module):
    """SqueezeNet's module: 1x1 squeeze-ReLU, then 1x1 and 3x3 pad-1 expands, each with ReLU, concatenated."""

    def __init__(self, cin, squeeze, e1, e3):
        super().__init__()
        self.squeeze = nn.Conv2d(cin, squeeze, 1)
        self.expand1x1 = nn.Conv2d(squeeze, e1, 1)
        self.expand3x3 = nn.Conv2d(squeeze, e3, 3, padding=1)

    def forward(self, x):
        s = F.relu(self.squeeze(x))
        return torch.cat([F.relu(self.expand1x1(s)), F.relu(self.expand3x3(s))], 1)


def _pool_ceil():
    return nn.MaxPool2d(3, 2, ceil_mode=True)


class SqueezeNet(nn.Module):
    """torchvision v0.10's squeezenet1_0 (1,248,424 parameters) / squeezenet1_1 (1,235,496): ceil-mode max
    pools, and a head that is a 1x1 conv to the classes, ReLU and a global average pool."""

    def __init__(self, version="1_0", num_classes=1000):
        super().__init__()
        self.version = version
        if version == "1_0":
            feats = [nn.Conv2d(3, 96, 7, 2), nn.ReLU(inplace=True), _pool_ceil(), Fire(96, 16, 64, 64),
                     Fire(128, 16, 64, 64), Fire(128, 32, 128, 128), _pool_ceil(), Fire(256, 32, 128, 128),
                     Fire(256, 48, 192, 192), Fire(384, 48, 192, 192), Fire(384, 64, 256, 256), _pool_ceil(),
                     Fire(512, 64, 256, 256)]
        elif version == "1_1":
            feats = [nn.Conv2d(3, 64, 3, 2), nn.ReLU(inplace=True), _pool_ceil(), Fire(64, 16, 64, 64),
                     Fire(128, 16, 64, 64), _pool_ceil(), Fire(128, 32, 128, 128), Fire(256, 32, 128, 128),
                     _pool_ceil(), Fire(256, 48, 192, 192), Fire(384, 48, 192, 192), Fire(384, 64, 256, 256),
                     Fire(512, 64, 256, 256)]
        else:
            raise ValueError(f"SqueezeNet version must be '1_0' or '1_1', got {version!r}")
        self.features = nn.Sequential(*feats)
        final = nn.Conv2d(512, num_classes, 1)
        self.classifier = nn.Sequential(nn.Dropout(0.5), final, nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d(1))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                if m is final:
                    nn.init.normal_(m.weight, 0.0, 0.01)
                else:
                    nn.init.kaiming_uniform_(m.weight)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return torch.flatten(self.classifier(self.features(x)), 1)


def squeezenet1_0(num_classes=1000):
    return SqueezeNet("1_0", num_classes)


def squeezenet1_1(num_classes=1000):
    return SqueezeNet("1_1", num_classes)


class DenseLayer(nn.Module):
    """torchvision's ``_DenseLayer``: BN -> ReLU -> 1x1 to 4 * growth -> BN -> ReLU -> 3x3 to growth."""

    def __init__(self, cin, growth, bn_size=4):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = _conv(cin, bn_size * growth, 1)
        self.norm2 = nn.BatchNorm2d(bn_size * growth)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = _conv(bn_size * growth, growth, 3, 1, 1)

    def forward(self, x):
        return self.conv2(self.relu2(self.norm2(self.conv1(self.relu1(self.norm1(x))))))


class DenseBlock(nn.Module):
    """``denselayer{j}`` children, each fed the concatenation of the block's input and every earlier layer's output."""

    def __init__(self, n, cin, growth):
        super().__init__()
        for j in range(n):
            self.add_module(f"denselayer{j + 1}", DenseLayer(cin + j * growth, growth))

    def forward(self, x):
        for layer in self.children():
            x = torch.cat([x, layer(x)], 1)
        return x


class DenseNet(nn.Module):
    """torchvision v0.10 DenseNet-BC (growth 32, bn_size 4, 64 stem channels, compression 0.5), its key names."""

    def __init__(self, block_config, growth=32, num_init=64, num_classes=1000):
        super().__init__()
        self.growth, self.block_config = growth, tuple(block_config)
        f = nn.Sequential()
        f.add_module("conv0", _conv(3, num_init, 7, 2, 3))
        f.add_module("norm0", nn.BatchNorm2d(num_init))
        f.add_module("relu0", nn.ReLU(inplace=True))
        f.add_module("pool0", nn.MaxPool2d(3, 2, 1))
        c = num_init
        for i, n in enumerate(block_config):
            f.add_module(f"denseblock{i + 1}", DenseBlock(n, c, growth))
            c += n * growth
            if i != len(block_config) - 1:
                t = nn.Sequential()
                t.add_module("norm", nn.BatchNorm2d(c))
                t.add_module("relu", nn.ReLU(inplace=True))
                t.add_module("conv", _conv(c, c // 2, 1))
                t.add_module("pool", nn.AvgPool2d(2, 2))
                f.add_module(f"transition{i + 1}", t)
                c //= 2
        f.add_module("norm5", nn.BatchNorm2d(c))
        self.features = f
        self.classifier = nn.Linear(c, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = F.relu(self.features(x))
        return self.classifier(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


def densenet121(num_classes=1000):
    return DenseNet((6, 12, 24, 16), num_classes=num_classes)


def densenet169(num_classes=1000):
    return DenseNet((6, 12, 32, 32), num_classes=num_classes)


def densenet201(num_classes=1000):
    return DenseNet((6, 12, 48, 32), num_classes=num_classes)


def channel_shuffle(x, groups=2):
    b, c, h, w = x.shape
    return x.view(b, groups, c // groups, h, w).transpose(1, 2).reshape(b, c, h, w)


class ShuffleUnit(nn.Module):
    """torchvision's ShuffleNetV2 ``InvertedResidual``.  ``branch2``: 1x1-BN-ReLU, depthwise 3x3-BN (no activation),
    1x1-BN-ReLU, on the second half of the channels at stride 1 and on all of them at stride 2; ``branch1``
    (stride 2 only): depthwise 3x3-BN, 1x1-BN-ReLU.  Concat, then ``channel_shuffle(2)``."""

    def __init__(self, cin, c, stride):
        super().__init__()
        h = c // 2
        self.stride = stride
        if stride == 1 and cin != c:
            raise ValueError("a stride-1 unit keeps its width")
        self.branch1 = nn.Sequential() if stride == 1 else nn.Sequential(
            _conv(cin, cin, 3, 2, 1, groups=cin), nn.BatchNorm2d(cin), _conv(cin, h, 1), nn.BatchNorm2d(h),
            nn.ReLU(inplace=True))
        self.branch2 = nn.Sequential(
            _conv(cin if stride == 2 else h, h, 1), nn.BatchNorm2d(h), nn.ReLU(inplace=True),
            _conv(h, h, 3, stride, 1, groups=h), nn.BatchNorm2d(h), _conv(h, h, 1), nn.BatchNorm2d(h),
            nn.ReLU(inplace=True))

    def forward(self, x):
        if self.stride == 1:
            x1, x2 = x.chunk(2, dim=1)
            out = torch.cat((x1, self.branch2(x2)), dim=1)
        else:
            out = torch.cat((self.branch1(x), self.branch2(x)), dim=1)
        return channel_shuffle(out, 2)


class ShuffleNetV2(nn.Module):
    """torchvision v0.10 ShuffleNetV2 (stages of 4, 8 and 4 units, 24-channel stem, 1024-wide conv5), its key names.
    Parameters keep PyTorch's default initialisation, as torchvision's do."""

    def __init__(self, widths, num_classes=1000):
        super().__init__()
        self.widths = tuple(widths)
        self.conv1 = nn.Sequential(_conv(3, 24, 3, 2, 1), nn.BatchNorm2d(24), nn.ReLU(inplace=True))
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 24
        for name, n, c in zip(("stage2", "stage3", "stage4"), (4, 8, 4), widths):
            setattr(self, name, nn.Sequential(*[ShuffleUnit(cin if i == 0 else c, c, 2 if i == 0 else 1)
                                                for i in range(n)]))
            cin = c
        self.conv5 = nn.Sequential(_conv(cin, 1024, 1), nn.BatchNorm2d(1024), nn.ReLU(inplace=True))
        self.fc = nn.Linear(1024, num_classes)

    def forward(self, x):
        x = self.maxpool(self.conv1(x))
        x = self.conv5(self.stage4(self.stage3(self.stage2(x))))
        return self.fc(x.mean(dim=(2, 3)))


def shufflenet_v2_x0_5(num_classes=1000):
    return ShuffleNetV2((48, 96, 192), num_classes)


def shufflenet_v2_x1_0(num_classes=1000):
    return ShuffleNetV2((116, 232, 464), num_classes)


def shufflenet_v2_x1_5(num_classes=1000):
    return ShuffleNetV2((176, 352, 704), num_classes)


def resnet18(num_classes=1000):
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes)


def resnet34(num_classes=1000):
    return ResNet(BasicBlock, [3, 4, 6, 3], num_classes)


def resnet50(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes)


def resnet101(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes)


def resnet152(num_classes=1000):
    return ResNet(Bottleneck, [3, 8, 36, 3], num_classes)


def resnext50_32x4d(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, groups=32, width_per_group=4)


def resnext101_32x8d(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes, groups=32, width_per_group=8)


def wide_resnet50_2(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes, width_per_group=128)


def wide_resnet101_2(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes, width_per_group=128)


def alexnet(num_classes=1000):
    return AlexNet(num_classes)


# torchvision v0.10's ResNet family (the hub the reference loads from) + AlexNet + MobileNetV2 / V3 + SqueezeNet +
# DenseNet + ShuffleNetV2 (not shufflenet_v2_x2_0: its 2048-wide conv5 is wider than conv1x1_narrow takes)
BUILDERS = {"resnet18": resnet18, "resnet34": resnet34, "resnet50": resnet50, "alexnet": alexnet,
            "resnet101": resnet101, "resnet152": resnet152, "resnext50_32x4d": resnext50_32x4d,
            "resnext101_32x8d": resnext101_32x8d, "wide_resnet50_2": wide_resnet50_2,
            "wide_resnet101_2": wide_resnet101_2, "mobilenet_v2": mobilenet_v2,
            "mobilenet_v3_large": mobilenet_v3_large, "mobilenet_v3_small": mobilenet_v3_small,
            "squeezenet1_0": squeezenet1_0, "squeezenet1_1": squeezenet1_1,
            "densenet121": densenet121, "densenet169": densenet169, "densenet201": densenet201,
            "shufflenet_v2_x0_5": shufflenet_v2_x0_5, "shufflenet_v2_x1_0": shufflenet_v2_x1_0,
            "shufflenet_v2_x1_5": shufflenet_v2_x1_5}

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def preprocess_u8(img_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [B,H,W,3] -> normalised fp32 NCHW (ToTensor + Normalize, reference
    alexnet_resnet.py:60-61)."""
    x = img_u8.permute(0, 3, 1, 2).float().div_(255.0)
    mean, std = _norm_consts(x.device)
    return (x - mean) / std


_NORM: dict = {}


def _norm_consts(device):
    """Per-device cached mean/std (no H2D copy inside a graph capture)."""
    key = str(device)
    if key not in _NORM:
        _NORM[key] = (torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1),
                      torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1))
    return _NORM[key]


_BUILD_LOCK = threading.Lock()


def build(name: str, seed: int = 0, randomize_bn: bool = False) -> nn.Module:
    """Random-init model of the named architecture, in eval mode.

    ``randomize_bn`` gives BN non-trivial affine params / running stats so the
    BN-folding path is actually exercised by the numerics tests.
    """
    name = canonical(name)
    g = torch.Generator().manual_seed(seed)
    # nn.init draws from the process-global CPU generator: nodes of one process
    # building models concurrently (LocalCluster threads) would interleave their
    # draws and get different weights for the same seed, so builds serialise.
    with _BUILD_LOCK, torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        m = BUILDERS[name]()
    if randomize_bn:
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                c = mod.num_features
                mod.weight.data = 0.5 + torch.rand(c, generator=g)
                mod.bias.data = 0.2 * torch.randn(c, generator=g)
                mod.running_mean.data = 0.2 * torch.randn(c, generator=g)
                mod.running_var.data = 0.5 + torch.rand(c, generator=g)
    return m.eval()


ALIASES = {"resnet": "resnet18", "resnet-18": "resnet18", "resnet_18": "resnet18",
           "resnet-50": "resnet50", "alex": "alexnet", "resnet-101": "resnet101", "resnet-152": "resnet152",
           "resnext50": "resnext50_32x4d", "resnext101": "resnext101_32x8d",
           "wide_resnet50": "wide_resnet50_2", "wide_resnet101": "wide_resnet101_2",
           "mobilenet": "mobilenet_v2", "mobilenetv2": "mobilenet_v2", "mobilenet-v2": "mobilenet_v2",
           "mobilenetv3_large": "mobilenet_v3_large", "mobilenet-v3-large": "mobilenet_v3_large",
           "mobilenet_v3": "mobilenet_v3_large", "mobilenetv3_small": "mobilenet_v3_small",
           "mobilenet-v3-small": "mobilenet_v3_small",
           "squeezenet": "squeezenet1_1", "squeezenet1.1": "squeezenet1_1", "squeezenet-1.1": "squeezenet1_1",
           "squeezenet1.0": "squeezenet1_0", "squeezenet-1.0": "squeezenet1_0",
           "densenet": "densenet121", "densenet-121": "densenet121", "densenet-169": "densenet169",
           "densenet-201": "densenet201",
           "shufflenet": "shufflenet_v2_x1_0", "shufflenet_v2": "shufflenet_v2_x1_0",
           "shufflenetv2_x0.5": "shufflenet_v2_x0_5", "shufflenetv2_x1.0": "shufflenet_v2_x1_0",
           "shufflenetv2_x1.5": "shufflenet_v2_x1_5", "shufflenetv2-x0.5": "shufflenet_v2_x0_5",
           "shufflenetv2-x1.0": "shufflenet_v2_x1_0", "shufflenetv2-x1.5": "shufflenet_v2_x1_5"}


def canonical(name: str) -> str:
    """Canonical model name; accepts ``resnet`` as an alias for ``resnet18``
    (the reference's shell help says "alexnet or resnet", mp4_machinelearning.py:1126,
    while its batch/stat keys use "resnet18", :646, 1106 — SURVEY.md A15)."""
    n = name.strip().lower()
    n = ALIASES.get(n, n)
    if n not in BUILDERS:
        raise ValueError(f"unknown model {name!r}; known: {sorted(BUILDERS)}")
    return n
