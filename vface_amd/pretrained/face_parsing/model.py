"""BiSeNet (ResNet-18 context path, feature fusion, three heads) as a parameter container with the reference's state-dict keys
(``REFace/pretrained/face_parsing/model.py``); ``vface_amd.parsing.ParseEngine`` executes it on the HIP kernels.

``conv_out16`` / ``conv_out32`` hold parameters so that checkpoints load, and are never run: ``FaceParser.forward`` keeps the first
of the three outputs only (face_parsing_demo.py:277).
"""
from typing import Optional

import torch
import torch.nn as nn

from ...convnet import EngineOwner
from .resnet import Resnet18

SEG_MEAN = (0.485, 0.456, 0.406)      # model.py:15-16; the pre-filter kernel holds the same constants
SEG_STD = (0.229, 0.224, 0.225)


class ConvBNReLU(nn.Module):
    def __init__(self, cin, cout, ks=3):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=ks, stride=1, padding=ks // 2, bias=False)
        self.bn = nn.BatchNorm2d(cout)


class BiSeNetOutput(nn.Module):
    def __init__(self, cin, cmid, n_classes):
        super().__init__()
        self.conv = ConvBNReLU(cin, cmid)
        self.conv_out = nn.Conv2d(cmid, n_classes, kernel_size=1, bias=False)


class AttentionRefinementModule(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = ConvBNReLU(cin, cout)
        self.conv_atten = nn.Conv2d(cout, cout, kernel_size=1, bias=False)
        self.bn_atten = nn.BatchNorm2d(cout)


class ContextPath(nn.Module):
    def __init__(self):
        super().__init__()
        self.resnet = Resnet18()
        self.arm16 = AttentionRefinementModule(256, 128)
        self.arm32 = AttentionRefinementModule(512, 128)
        self.conv_head32 = ConvBNReLU(128, 128)
        self.conv_head16 = ConvBNReLU(128, 128)
        self.conv_avg = ConvBNReLU(512, 128, ks=1)


class FeatureFusionModule(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.convblk = ConvBNReLU(cin, cout, ks=1)
        self.conv1 = nn.Conv2d(cout, cout // 4, kernel_size=1, bias=False)
        self.conv2 = nn.Conv2d(cout // 4, cout, kernel_size=1, bias=False)


class BiSeNet(EngineOwner, nn.Module):
    def __init__(self, n_classes: int = 19, compute_dtype: torch.dtype = torch.float16):
        super().__init__()
        self.cp = ContextPath()
        self.ffm = FeatureFusionModule(256, 256)
        self.conv_out = BiSeNetOutput(256, 256, n_classes)
        self.conv_out16 = BiSeNetOutput(128, 64, n_classes)
        self.conv_out32 = BiSeNetOutput(128, 64, n_classes)
        self.n_classes = n_classes
        self.compute_dtype = compute_dtype
        self.eval()

    def _make_engine(self):
        from ...parsing import ParseEngine
        return ParseEngine(self.state_dict(), self.compute_dtype, next(self.parameters()).device)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, size: Optional[tuple] = None) -> torch.Tensor:
        """Normalised images [N, 3, H, W] on the device -> the class logits at H/8 x W/8, fp32 [N, n_classes, H/8, W/8]: the
        tensor the reference upsamples (model.py:258).  The upsampled planes are never built here; ``FaceParser.labels`` goes
        from these logits to the label bytes in one kernel."""
        N, _, H, W = x.shape
        low = self.engine.logits(self.engine.tokens8(x), N, H, W)
        return low.view(N, H // 8, W // 8, -1)[..., :self.n_classes].permute(0, 3, 1, 2).contiguous()
