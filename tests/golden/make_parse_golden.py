#!/usr/bin/env python3
"""Writes tests/golden/parse.npz: the REFERENCE's own outputs for the face-parsing path, recorded by running its
``pretrained/face_parsing`` -- ``BiSeNet`` (fp32, ``.double()`` and ``.half()`` on the CPU), ``BicubicDownSample(factor=2,
cuda=False)`` and ``__ffhq_masks_to_faceParser_mask_detailed`` -- on the inputs of cases_parse.py with the name-keyed weights of
``vface_amd.utils.synth.fill_parser_``.  Only arrays and name lists are written.

    python tests/golden/make_parse_golden.py /path/to/REFace

Three things the reference does at import or construction are neutralised BEFORE they run:
  1. ``Resnet18.__init__`` fetches ImageNet weights from a URL (resnet.py:82-88): ``init_weight`` becomes a no-op and the two
     download functions raise, before any ``BiSeNet`` is built;
  2. model.py:15-16 calls ``.cuda()`` at import: ``torch.Tensor.cuda`` is the identity for this run;
  3. ``torchvision`` and ``cv2`` are imported and not used on these paths: empty stand-in modules.

Per network input size ``HxW`` of cases_parse.NET_SIZES the file holds ``HxW.logits32`` (the ``conv_out`` module's output, taken
with a forward hook: 19 x H/8 x W/8), ``HxW.logits64`` (the same from the ``.double()`` run; at 512 x 512 stored rounded to fp32,
a relative 6e-8 against a yardstick of 5e-3, to keep the file small), ``HxW.e_ref`` (max |half run - double run| of those logits),
``HxW.labels19`` / ``HxW.labels12`` and, for the two small sizes, ``HxW.prefilter`` (``preprocess_img``'s tensor).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import cases_parse as cp  # noqa: E402
from vface_amd.utils import synth  # noqa: E402


def load_reference(root: str):
    for name in ("torchvision", "cv2"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)

    def refuse(*a, **k):
        raise RuntimeError("the fixture never downloads anything")
    import torch.hub
    import torch.utils.model_zoo
    torch.utils.model_zoo.load_url = refuse
    torch.hub.load_state_dict_from_url = refuse
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, root)
    from pretrained.face_parsing import resnet
    resnet.Resnet18.init_weight = lambda self: None
    resnet.modelzoo.load_url = refuse
    from pretrained.face_parsing import face_parsing_demo as demo
    from pretrained.face_parsing import model
    return demo, model


@torch.no_grad()
def main():
    demo, model = load_reference(sys.argv[1])
    seg12 = getattr(demo, "__ffhq_masks_to_faceParser_mask_detailed")
    net = model.BiSeNet(n_classes=cp.N_CLASSES).eval()
    synth.fill_parser_(net, seed=cp.WEIGHT_SEED)
    sd = net.state_dict()
    out = {"keys": np.array(list(sd.keys())), "shapes": np.array([",".join(str(s) for s in v.shape) for v in sd.values()]),
           "seg12_of_arange": seg12(np.arange(256, dtype=np.uint8)), "torch_version": np.array(torch.__version__)}
    down = demo.BicubicDownSample(factor=2, cuda=False)
    got = {}
    nets = {}
    for dt in (torch.float32, torch.float64, torch.float16):      # three networks from the SAME fp32 weights (a .half().float() round
        nets[dt] = model.BiSeNet(n_classes=cp.N_CLASSES).eval()   # trip on one module would leave it with rounded parameters)
        nets[dt].load_state_dict(sd)
        nets[dt].to(dt)
        nets[dt].conv_out.register_forward_hook(lambda m, i, o: got.__setitem__("low", o.detach().clone()))
    for (H, W) in cp.NET_SIZES:
        tag = f"{H}x{W}"
        u8 = torch.from_numpy(cp.crop(H, W, cp.SEEDS[(H, W)]))
        im = (u8.permute(2, 0, 1).float().div(255))[None]                      # ToTensor
        x = (down(im).clamp(0, 1) - model.seg_mean) / model.seg_std            # preprocess_img, :264
        full, _, _ = nets[torch.float32](x)
        low32 = got["low"][0]
        lab = torch.argmax(full, dim=1)[0].numpy().astype(np.uint8)            # forward :278, faceParsing_demo :305
        nets[torch.float64](x.double())
        low64 = got["low"][0]
        nets[torch.float16](x.half())
        e_ref = float((got["low"][0].double() - low64).abs().max())
        if H * W <= 96 * 64:
            out[f"{tag}.prefilter"] = x[0].numpy()
        out[f"{tag}.logits32"] = low32.numpy()
        out[f"{tag}.logits64"] = low64.numpy() if H * W <= 96 * 64 else low64.float().numpy()
        out[f"{tag}.e_ref"] = np.array(e_ref)
        out[f"{tag}.labels19"] = lab
        out[f"{tag}.labels12"] = seg12(lab)
        print(tag, "e_ref", e_ref, "logit std", float(low64.std()), "labels", np.unique(lab).tolist(), flush=True)
    path = os.path.join(HERE, "parse.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
