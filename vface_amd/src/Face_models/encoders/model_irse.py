"""ArcFace ``Backbone`` (IR-SE50) as a parameter container with the reference's state-dict keys
(``REFace/src/Face_models/encoders/{model_irse,helpers}.py``); ``vface_amd.arcface.ArcFaceEngine`` executes it on the HIP kernels.

Only what ``IDLoss`` builds is shipped: ``input_size=112, num_layers=50, mode='ir_se'``, single scale.  ``Dropout`` and ``Flatten``
hold no parameters: they are placeholders that keep ``output_layer``'s indices (0, 3, 4).
"""
import torch
import torch.nn as nn

from ....arcface import SE_REDUCTION, UNITS, check_config
from ....convnet import EngineOwner


class SEModule(nn.Module):
    def __init__(self, channels: int, reduction: int):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1, bias=False)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1, bias=False)


class bottleneck_IR_SE(nn.Module):
    def __init__(self, in_channel: int, depth: int, stride: int):
        super().__init__()
        if in_channel == depth:
            self.shortcut_layer = nn.Identity()      # MaxPool2d(1, stride): no parameters
        else:
            self.shortcut_layer = nn.Sequential(nn.Conv2d(in_channel, depth, 1, stride, bias=False), nn.BatchNorm2d(depth))
        self.res_layer = nn.Sequential(nn.BatchNorm2d(in_channel), nn.Conv2d(in_channel, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                                       nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth),
                                       SEModule(depth, SE_REDUCTION))


class Backbone(EngineOwner, nn.Module):
    def __init__(self, input_size: int = 112, num_layers: int = 50, mode: str = "ir_se", drop_ratio: float = 0.4, affine: bool = True,
                 compute_dtype: torch.dtype = torch.float16):
        super().__init__()
        check_config(input_size, num_layers, mode)
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(512), nn.Identity(), nn.Identity(), nn.Linear(512 * 7 * 7, 512),
                                          nn.BatchNorm1d(512, affine=affine))
        self.body = nn.Sequential(*[bottleneck_IR_SE(*u) for u in UNITS])
        self.compute_dtype = compute_dtype
        self.eval()

    def _make_engine(self):
        from ....arcface import ArcFaceEngine
        return ArcFaceEngine(self.state_dict(), self.compute_dtype, next(self.parameters()).device)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, multi_scale: bool = False):
        """Images [B, 3, 112, 112] on the device -> ``[features]``, fp32 [B, 512] rows of unit length."""
        check_config(multi_scale=multi_scale)
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, 112, 112):
            raise NotImplementedError(f"the identity network takes [B, 3, 112, 112]; got {tuple(x.shape)}")
        return [self.engine.features(self.engine.tokens8(x), x.shape[0])]
