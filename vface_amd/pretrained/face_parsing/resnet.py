"""ResNet-18 trunk of the face parser as a parameter container (``REFace/pretrained/face_parsing/resnet.py``).

The state-dict keys are the reference's (``conv1``, ``bn1``, ``layer1..4.{0,1}.{conv1,bn1,conv2,bn2,downsample.{0,1}}``), so a
face-parsing checkpoint loads with ``load_state_dict``.  There is no ``init_weight``: the reference's fetches ImageNet weights from
a URL at construction, which a checkpoint overwrites anyway.  Execution is ``vface_amd.parsing.ParseEngine``; nothing here computes.
"""
import torch.nn as nn


def _conv(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=False)


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.conv1, self.bn1 = _conv(cin, cout, 3, stride), nn.BatchNorm2d(cout)
        self.conv2, self.bn2 = _conv(cout, cout, 3), nn.BatchNorm2d(cout)
        self.downsample = None
        if cin != cout or stride != 1:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))


class Resnet18(nn.Module):
    WIDTHS = (64, 128, 256, 512)

    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = _conv(3, 64, 7, 2), nn.BatchNorm2d(64)
        cin = 64
        for li, cout in enumerate(self.WIDTHS, start=1):
            setattr(self, f"layer{li}", nn.Sequential(BasicBlock(cin, cout, 1 if li == 1 else 2), BasicBlock(cout, cout)))
            cin = cout
