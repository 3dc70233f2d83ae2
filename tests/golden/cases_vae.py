"""What tests/golden/make_golden.py::gen_vae_stages and the tests that read tests/golden/vae_stages.npz share: the two cases, their
seeded inputs, the names of the stages ``VAEEngine`` sequences (its own packed-weight keys) and WHICH ELEMENTS of a stage output the
fixture holds.  A whole fp64 intermediate of ``ragged`` is 0.5 M values and there are 39 of them, so the fixture keeps, per stage,
``K_STAGE`` seeded elements of the NCHW-flattened output (all of it where it is smaller) as the fp64 run's value rounded to fp32, and
``K_DEC`` elements of the decoded images; latent-sized outputs are whole.  Every comparison -- the oracle's, the CPU model's, the
engine's -- is made on the same elements, so the figures are comparable with each other; none is a whole-tensor norm."""
import zlib

import numpy as np

DD = {"small": dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
                    attn_resolutions=[], dropout=0.0),
      "ffhq": dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
                   attn_resolutions=[], dropout=0.0)}
CASES = {"ragged": dict(cfg="small", frames=2, H=80, W=96),      # latent 10 x 12: n = 120, % 8 == 0, % 64 != 0
         "wide": dict(cfg="ffhq", frames=1, H=192, W=256)}       # latent 24 x 32: n = 768, twelve key tiles, c = 512
SCALE = 0.18215
K_STAGE, K_DEC = 2048, 8192
AUTOCAST = {"ragged": ("f16", "bf16"), "wide": ("f16", "bf16")}  # the types whose reference autocast run is recorded


def inputs(case):
    """``(x [F, 3, H, W] in [-1, 1], noise [F, 4, H / 8, W / 8])``, fp32 torch tensors."""
    from vface_amd.utils import synth
    c = CASES[case]
    x = synth.synth_normal(f"vae.{case}.x", (c["frames"], 3, c["H"], c["W"])).clamp(-1, 1)
    return x, synth.synth_normal(f"vae.{case}.noise", (c["frames"], 4, c["H"] // 8, c["W"] // 8))


def enc_stages(nres=4, nrb=2):
    out = ["enc.conv_in"]
    for lvl in range(nres):
        out += [f"enc.down.{lvl}.{b}" for b in range(nrb)]
        if lvl != nres - 1:
            out.append(f"enc.down.{lvl}.ds")
    return out + ["enc.mid1", "enc.attn", "enc.mid2"]           # then ``moments`` = norm_out + conv_out + quant_conv, whole


def dec_stages(nres=4, nrb=2):
    out = ["dec.conv_in", "dec.mid1", "dec.attn", "dec.mid2"]   # dec.conv_in: post_quant_conv + conv_in
    for lvl in reversed(range(nres)):
        out += [f"dec.up.{lvl}.{b}" for b in range(nrb + 1)]
        if lvl != 0:
            out.append(f"dec.up.{lvl}.us")
    return out                                                  # then ``dec`` = norm_out + conv_out, K_DEC elements


def pick(name, numel, k):
    """The sorted flat indices kept of an output of ``numel`` elements (None: all of it)."""
    if numel <= k:
        return None
    return np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(numel, k, replace=False))


def take(case, stage, t, k=K_STAGE):
    """The fixture's elements of the NCHW tensor ``t`` (torch), flat."""
    import torch
    idx = pick(f"{case}.{stage}", t.numel(), k)
    flat = t.reshape(-1)
    return flat if idx is None else flat[torch.from_numpy(idx)]
