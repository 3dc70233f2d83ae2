"""The face-parsing network on the HIP kernels: aligned crop -> label map, without leaving the GPU.

``REFace/scripts/VFace_inference_batch.py:251, 292-294`` calls ``faceParsing_demo`` -> ``FaceParser.forward`` -> ``BiSeNet`` over
``Resnet18`` (``pretrained/face_parsing/{face_parsing_demo,model,resnet}.py``) once per frame, in fp32, with a host round trip.
``ParseEngine`` runs the same network for a whole batch of frames, on ``convnet.ConvNetEngine`` as ``RaftEngine`` does:

  * eval-mode BatchNorm (eps 1e-5) is folded into every convolution on the host, in fp64 (all of them are bias-free, the ResNet's
    ``downsample.1`` and the gates' ``bn_atten`` included);
  * the 7x7 stride-2 stem and the strided 1x1 shortcuts go through ``vface_im2col`` + ``vface_gemm``, every 3x3 through
    ``vface_conv3x3`` (the nearest x2 upsampling in front of ``conv_head32`` / ``conv_head16`` is its ``upsample`` form), ReLUs
    and residual adds through ``vface_channel_norm_act``; 16-bit operands, fp32 accumulation;
  * the global average pools are the means ``vface_channel_stats`` leaves behind; the 1x1 convolutions on those pooled vectors,
    their folded BatchNorm and ReLU / sigmoid are ``vface_pooled_linear`` (fp32 end to end: a gate is 128 or 256 numbers per image);
  * max-pool, the gates with the add that follows each, the pre-filter and the head are the kernels of ``csrc/parsing.hip``.  The
    class head is padded 19 -> 32 columns and written in fp32; ``vface_upsample_argmax_u8`` turns it into one byte per pixel.

``conv_out16`` / ``conv_out32`` and their upsamplings are not run: ``FaceParser.forward`` discards them (``down_seg, _, _``), so the
result is the same.  Their state-dict keys are accepted and ignored.  ``split_k = False`` keeps the ``window`` launches (im2col +
``vface_gemm``) from splitting K, a choice that is made from M and so from the batch; the 3x3 launches do follow the split-K rules of
``vface_conv3x3``, which read the per-sample geometry (rows per image, channels) only.  No kernel uses atomics, so a frame's label map
does not depend on which frames share its batch.  No CPU fallback: without the HIP library every call raises.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import hip
from .convnet import ConvNetEngine, fold_bn      # (fold_bn: re-exported, the CPU restatement of the network folds with it)

N_CLASSES = 19
HEAD_COLS = 32                       # the class head's padded width = the byte table's length
LAYERS = ((64, 1), (128, 2), (256, 2), (512, 2))      # ResNet-18: (width, stride of the first block) of layer1..4
BN_EPS = 1e-5

# `__ffhq_masks_to_faceParser_mask_detailed` (face_parsing_demo.py:74-122) as a table: 19 labels -> 12; a label it does not name
# maps to 0, as its zero-initialised output does.
_SEG12 = {0: 0, 12: 1, 13: 1, 2: 2, 3: 2, 4: 3, 5: 3, 17: 4, 10: 5, 1: 6, 7: 7, 8: 7, 14: 8, 11: 9, 6: 10, 9: 11}


def seg12_table() -> torch.Tensor:
    """uint8 [32]: entry v = the 12-class label of 19-class label v."""
    t = torch.zeros(HEAD_COLS, dtype=torch.uint8)
    for k, v in _SEG12.items():
        t[k] = v
    return t


def identity_table() -> torch.Tensor:
    return torch.arange(HEAD_COLS, dtype=torch.uint8)


class ParseEngine(ConvNetEngine):
    """Executes ``BiSeNet(n_classes=19)`` on device buffers.  ``sd``: its state dict (any float dtype, any device)."""
    split_k = False      # a frame's labels must not depend on its batch (see ConvNetEngine.split_k)

    def __init__(self, sd: Dict[str, torch.Tensor], dtype: torch.dtype = torch.float16, device="cuda:0",
                 window_budget_bytes: int = 256 << 20):
        super().__init__(dtype, device)
        self.window_budget = window_budget_bytes
        sd = {k: v.detach().double().cpu() for k, v in sd.items() if torch.is_floating_point(v)}      # BatchNorm is folded in fp64
        r = "cp.resnet"
        self.add_conv(sd, f"{r}.conv1", f"{r}.bn1", cin_pad=8)
        for li in range(1, 5):
            for bi in (0, 1):
                b = f"{r}.layer{li}.{bi}"
                self.add_conv(sd, f"{b}.conv1", f"{b}.bn1")
                self.add_conv(sd, f"{b}.conv2", f"{b}.bn2")
                if f"{b}.downsample.0.weight" in sd:
                    self.add_conv(sd, f"{b}.downsample.0", f"{b}.downsample.1")
        for arm in ("cp.arm16", "cp.arm32"):
            self.add_conv(sd, f"{arm}.conv.conv", f"{arm}.conv.bn")
            self.add_conv(sd, f"{arm}.conv_atten", f"{arm}.bn_atten", pooled=True)
        self.add_conv(sd, "cp.conv_avg.conv", "cp.conv_avg.bn", pooled=True)
        self.add_conv(sd, "cp.conv_head32.conv", "cp.conv_head32.bn")
        self.add_conv(sd, "cp.conv_head16.conv", "cp.conv_head16.bn")
        self.add_conv(sd, "ffm.convblk.conv", "ffm.convblk.bn")
        self.add_conv(sd, "ffm.conv1", pooled=True)
        self.add_conv(sd, "ffm.conv2", pooled=True)
        self.add_conv(sd, "conv_out.conv.conv", "conv_out.conv.bn")
        self.add_conv(sd, "conv_out.conv_out", cout_pad=HEAD_COLS)
        self.n_classes = int(sd["conv_out.conv_out.weight"].shape[0])
        if self.n_classes > HEAD_COLS:
            raise hip.VFaceHipError(f"the class head holds at most {HEAD_COLS} classes; got {self.n_classes}")
        self.tables = {True: seg12_table().to(self.dev), False: identity_table().to(self.dev)}

    # ---- building blocks -------------------------------------------------------------------------------------------------
    def _relu(self, x, *, M, hw, C_, residual=None, y=None):
        hip.channel_norm_act(x, y if y is not None else x, M=M, hw=hw, C_=C_, act=hip.ACT_RELU, residual=residual)

    def _pooled(self, name, a, *, nimg, lda, sa, act):
        p = self.P[name]
        out = torch.empty(nimg, p["cout"], dtype=torch.float32, device=self.dev)
        hip.pooled_linear(a, p["w"], p["b"], out, nimg=nimg, N=p["cout"], K=p["cin"], lda=lda, sa=sa, act=act)
        return out

    def _means(self, x, *, nimg, hw, C_):
        """Global average pool: fp32 [nimg, C, 2] whose [..., 0] is the mean (``vface_channel_stats``)."""
        return hip.channel_stats(x, nimg=nimg, hw=hw, C_=C_)

    def _arm(self, arm, x, *, nimg, H, W, cin, rvec=None, rten=None, tap=None):
        """AttentionRefinementModule (model.py:82-89) and the add that follows it (:122 / :127), in place in its output.  ``tap`` as in
        ``logits``: ``<arm>.conv``, ``<arm>.conv.act``, ``<arm>.mean``, ``<arm>.conv_atten`` (the gate), ``<arm>.out`` (the gated sum)."""
        hw, M = H * W, nimg * H * W
        feat = self._buf(M, 128)
        self.conv3(f"{arm}.conv.conv", x, feat, nimg=nimg, H=H, W=W, ldx=cin)
        if tap:
            tap(f"{arm}.conv", feat)
        self._relu(feat, M=M, hw=hw, C_=128)
        if tap:
            tap(f"{arm}.conv.act", feat)
        m = self._means(feat, nimg=nimg, hw=hw, C_=128)
        if tap:
            tap(f"{arm}.mean", m)
        g = self._pooled(f"{arm}.conv_atten", m, nimg=nimg, lda=256, sa=2, act=hip.ACT_SIGMOID)
        if tap:
            tap(f"{arm}.conv_atten", g)
        hip.channel_gate(feat, g, feat, M=M, hw=hw, C_=128, rvec=rvec, rten=rten)
        if tap:
            tap(f"{arm}.out", feat)
        return feat

    # ---- the network -----------------------------------------------------------------------------------------------------
    @staticmethod
    def check_size(H: int, W: int):
        if H % 32 or W % 32 or min(H, W) < 64:
            raise hip.VFaceHipError(f"the face parser's input must be a multiple of 32 and at least 64 in both directions; got {H} x {W}")

    @torch.no_grad()
    def logits(self, x8: torch.Tensor, F: int, H: int, W: int, tap=None) -> torch.Tensor:
        """Token rows [F*H*W, 8] of the normalised input -> fp32 class logits [F * H/8 * W/8, 32] (columns 19..31 are zero).

        ``tap(name, tensor)`` (tests; production passes None) is called right after the launch that completes ``tensor``; it changes
        no launch, buffer or flag.  Buffers are reused and written in place: a tap that keeps must clone.  With r = ``cp.resnet`` and
        b = ``cp.resnet.layerL.B`` the names are
          ``x8`` (the input), ``r.conv1`` (after the last frame chunk), ``r.conv1.act``, ``r.maxpool``;
          ``b.conv1``, ``b.conv1.act``, ``b.conv2``, ``b.downsample.0`` (where present), ``b.sum`` (the ReLU of shortcut + residual),
          ``b.out`` (what the next block reads: the same rows);
          ``cp.avg.mean`` (fp32 [F, 512, 2]: [..., 0] is the mean), ``cp.conv_avg`` (fp32 [F, 128]);
          ``cp.arm32.conv``, ``.conv.act``, ``.mean``, ``.conv_atten``, ``.out``; the same under ``cp.arm16`` (``_arm``);
          ``cp.conv_head32``, ``cp.conv_head32.act``, ``cp.conv_head16``, ``cp.conv_head16.act`` (the right half of ``cat``);
          ``ffm.cat`` (all 256 columns), ``ffm.convblk``, ``ffm.convblk.act``, ``ffm.mean``, ``ffm.conv1``, ``ffm.conv2``, ``ffm.out``;
          ``conv_out.conv``, ``conv_out.conv.act``, ``logits`` (fp32 [M, 32])."""
        self.check_size(H, W)
        if not x8.is_cuda:
            raise hip.VFaceHipError("the face parser runs on the GPU: its input must be a device tensor (no CPU fallback)")
        if x8.dtype != self.dtype or tuple(x8.shape) != (F * H * W, 8) or not x8.is_contiguous():
            raise hip.VFaceHipError(f"logits: input must be contiguous {self.dtype} [{F * H * W}, 8]; got {x8.dtype} {tuple(x8.shape)}")
        if tap:
            tap("x8", x8)
        r = "cp.resnet"
        # stem: 7x7 stride 2 (+ folded bn1) -> ReLU -> max-pool.  The window matrix is 392 x 2 bytes per output pixel (51 MB per
        # 512 x 512 frame): built for a bounded number of frames at a time
        h2, w2 = H // 2, W // 2
        x = self._buf(F * h2 * w2, 64)
        per_frame = h2 * w2 * 392 * 2
        step = max(1, min(F, self.window_budget // per_frame))
        for f0 in range(0, F, step):
            n = min(step, F - f0)
            self.window(f"{r}.conv1", x8[f0 * H * W:(f0 + n) * H * W], x[f0 * h2 * w2:(f0 + n) * h2 * w2], nimg=n, H=H, W=W, C_=8, ldx=8,
                        stride=2)
        if tap:
            tap(f"{r}.conv1", x)
        self._relu(x, M=F * h2 * w2, hw=h2 * w2, C_=64)
        if tap:
            tap(f"{r}.conv1.act", x)
        h, w = h2 // 2, w2 // 2
        t = self._buf(F * h * w, 64)
        hip.maxpool3x3s2(x, t, nimg=F, H=h2, W=w2, C_=64)
        if tap:
            tap(f"{r}.maxpool", t)
        x, cin = t, 64
        feats = {}
        cat = None
        for li, (cout, stride) in enumerate(LAYERS, start=1):
            for bi in (0, 1):
                b = f"{r}.layer{li}.{bi}"
                st = stride if bi == 0 else 1
                c0 = cin if bi == 0 else cout
                oh, ow = (h - 1) // st + 1, (w - 1) // st + 1
                M = F * oh * ow
                t = self._buf(M, cout)
                self.conv3(f"{b}.conv1", x, t, nimg=F, H=h, W=w, ldx=x.stride(0), stride=st)
                if tap:
                    tap(f"{b}.conv1", t)
                self._relu(t, M=M, hw=oh * ow, C_=cout)
                if tap:
                    tap(f"{b}.conv1.act", t)
                t2 = self._buf(M, cout)
                self.conv3(f"{b}.conv2", t, t2, nimg=F, H=oh, W=ow, ldx=cout)
                if tap:
                    tap(f"{b}.conv2", t2)
                if li == 2 and bi == 1:      # feat8 is the left half of the fusion module's input [feat8 | feat_cp8]
                    cat = self._buf(M, 256)
                    y = cat[:, :128]
                else:
                    y = t2
                if f"{b}.downsample.0" in self.P:      # relu(bn(conv1x1 stride s (x)) + residual)
                    s = self._buf(M, cout)
                    self.window(f"{b}.downsample.0", x, s, nimg=F, H=h, W=w, C_=c0, ldx=x.stride(0), stride=st)
                    if tap:
                        tap(f"{b}.downsample.0", s)
                    self._relu(s, M=M, hw=oh * ow, C_=cout, residual=t2, y=y)
                else:                                      # relu(x + residual)
                    self._relu(x, M=M, hw=oh * ow, C_=cout, residual=t2, y=y)
                if tap:
                    tap(f"{b}.sum", y)
                x = y
                if tap:
                    tap(f"{b}.out", x)
                h, w = oh, ow
            cin = cout
            feats[li] = (x, h, w)
        (f8, h8, w8), (f16, h16, w16), (f32_, h32, w32) = feats[2], feats[3], feats[4]
        # context path (model.py:110-131)
        m32 = self._means(f32_, nimg=F, hw=h32 * w32, C_=512)
        if tap:
            tap("cp.avg.mean", m32)
        avg = self._pooled("cp.conv_avg.conv", m32, nimg=F, lda=1024, sa=2, act=hip.ACT_RELU)
        if tap:
            tap("cp.conv_avg", avg)
        s32 = self._arm("cp.arm32", f32_, nimg=F, H=h32, W=w32, cin=512, rvec=avg, tap=tap)   # feat32_arm + avg_up
        up32 = self._buf(F * h16 * w16, 128)
        self.conv3("cp.conv_head32.conv", s32, up32, nimg=F, H=h32, W=w32, ldx=128, upsample=True)
        if tap:
            tap("cp.conv_head32", up32)
        self._relu(up32, M=F * h16 * w16, hw=h16 * w16, C_=128)
        if tap:
            tap("cp.conv_head32.act", up32)
        s16 = self._arm("cp.arm16", f16, nimg=F, H=h16, W=w16, cin=256, rten=up32, tap=tap)   # feat16_arm + feat32_up
        M8 = F * h8 * w8
        self.conv3("cp.conv_head16.conv", s16, cat[:, 128:], nimg=F, H=h16, W=w16, ldx=128, upsample=True)
        if tap:
            tap("cp.conv_head16", cat[:, 128:])
        hip.channel_norm_act(cat[:, 128:], cat[:, 128:], M=M8, hw=h8 * w8, C_=128, act=hip.ACT_RELU, ldx=256, ldy=256)
        if tap:
            tap("cp.conv_head16.act", cat[:, 128:])
            tap("ffm.cat", cat)
        # feature fusion (:206-216): feat * atten + feat
        feat = self._buf(M8, 256)
        self.window("ffm.convblk.conv", cat, feat, nimg=F, H=h8, W=w8, C_=256, ldx=256)
        if tap:
            tap("ffm.convblk", feat)
        self._relu(feat, M=M8, hw=h8 * w8, C_=256)
        if tap:
            tap("ffm.convblk.act", feat)
        m8 = self._means(feat, nimg=F, hw=h8 * w8, C_=256)
        if tap:
            tap("ffm.mean", m8)
        a1 = self._pooled("ffm.conv1", m8, nimg=F, lda=512, sa=2, act=hip.ACT_RELU)
        if tap:
            tap("ffm.conv1", a1)
        a2 = self._pooled("ffm.conv2", a1, nimg=F, lda=64, sa=1, act=hip.ACT_SIGMOID)
        if tap:
            tap("ffm.conv2", a2)
        hip.channel_gate(feat, a2, feat, M=M8, hw=h8 * w8, C_=256, add_x=True)
        if tap:
            tap("ffm.out", feat)
        # head (:50-53): 3x3 + ReLU, then the 1x1 to the classes, fp32
        mid = self._buf(M8, 256)
        self.conv3("conv_out.conv.conv", feat, mid, nimg=F, H=h8, W=w8, ldx=256)
        if tap:
            tap("conv_out.conv", mid)
        self._relu(mid, M=M8, hw=h8 * w8, C_=256)
        if tap:
            tap("conv_out.conv.act", mid)
        out = torch.empty(M8, HEAD_COLS, dtype=torch.float32, device=self.dev)
        self.window("conv_out.conv_out", mid, out, nimg=F, H=h8, W=w8, C_=256, ldx=256, out32=True)
        if tap:
            tap("logits", out)
        return out

    @torch.no_grad()
    def prefilter(self, crops_u8: torch.Tensor) -> torch.Tensor:
        """uint8 crops [F, 2H, 2W, 3] -> token rows [F*H*W, 8] (``FaceParser.preprocess_img`` with the factor-2 filter)."""
        if not crops_u8.is_cuda:
            raise hip.VFaceHipError("the face parser runs on the GPU: crops must be device tensors (no CPU fallback)")
        F, H2, W2, _ = crops_u8.shape
        out = self._buf(F * (H2 // 2) * (W2 // 2), 8)
        hip.parse_prefilter(crops_u8, out, 2)
        return out

    @torch.no_grad()
    def labels(self, crops_u8: torch.Tensor, convert_to_seg12: bool = True) -> torch.Tensor:
        """uint8 crops [F, 2H, 2W, 3] on the device -> uint8 label maps [F, H, W] (12 classes, or the network's 19)."""
        if crops_u8.dim() != 4 or crops_u8.shape[3] != 3 or crops_u8.dtype != torch.uint8:
            raise hip.VFaceHipError(f"labels: crops must be uint8 [F, H, W, 3]; got {crops_u8.dtype} {tuple(crops_u8.shape)}")
        F, H2, W2, _ = crops_u8.shape
        if H2 % 2 or W2 % 2:
            raise hip.VFaceHipError(f"labels: the crops' size must be even; got {H2} x {W2}")
        H, W = H2 // 2, W2 // 2
        self.check_size(H, W)
        low = self.logits(self.prefilter(crops_u8.contiguous()), F, H, W)
        return hip.upsample_argmax_u8(low, self.tables[bool(convert_to_seg12)], F=F, h=H // 8, w=W // 8, ncls=self.n_classes, H=H, W=W)
