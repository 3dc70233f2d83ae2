"""ctypes binding of ``libvface_hip.so`` (C ABI: ``include/vface_hip.h``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every call below hands raw device
pointers and ``torch.cuda.current_stream().cuda_stream`` to a hand-written gfx950 kernel.  There is no
fallback: if the library is missing, or a tensor is not on the GPU, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (VFACE_HIP_LIB: another build of the same library, for A/B timing of two builds in one process tree; still the C ABI,
#  still no fallback: a path that does not load raises)
LIB_PATH = os.environ.get("VFACE_HIP_LIB") or os.path.join(_HERE, "lib", "libvface_hip.so")

F16, BF16 = 0, 1
EPI_GEGLU, EPI_OUT_F32 = 1, 2
CONV_PAD_TRAILING = 0x40000  # conv3x3: zero padding (0,1,0,1) (the VAE encoder's Downsample)
TUNE_NO_XCD_REMAP, TUNE_NO_SETPRIO = 0x1000, 0x2000  # A/B: gemm tiles in launch order / no raised wave priority around the MFMAs (conv.hip: split load issue)
TUNE_STAMPS = 0x4000  # diagnostic: the stamped instantiation; `colstats` receives cycle counts (tools/stamp_gemm.py, tools/stamp_conv.py)
TUNE_NARROW_EPILOGUE = 0x8000  # A/B: gemm.hip stores from the accumulator layout, no LDS transpose
TUNE_NO_PATCH, TUNE_PATCH = 0x80000, 0x100000  # conv3x3*: never / always (where the shape allows) the patch-staged kernel
TUNE_GN8 = 0x8000000  # A/B: fixed 8-wide column groups in the plain GEMM's tile order
TUNE_NO_Q8 = 0x4000000  # A/B: the 8x8 level stays on the im2col kernel
TUNE_PATCH_BN160 = 0x2000000  # A/B: patch kernel's 160-wide tile wherever it divides Cout
TUNE_F32_TRANSPOSE = 0x1000000  # A/B: epilogue transposes through LDS in fp32 even where 16 bits would do
TUNE_NO_PERSISTENT, TUNE_PERSISTENT = 0x10000, 0x20000  # flags of gemm / conv3x3: force one workgroup per tile / the persistent form
TUNE_BIG_W256, TUNE_BIG_W320 = 0x200000, 0x400000  # gemm, big tile: force the 256- / the 320-channel width (default: by grid rounds; same bits)
TUNE_BIG_TILE, TUNE_NO_BIG_TILE = 0x10000000, 0x20000000  # gemm: always (where the launch qualifies) / never the 256 x 320 tile (csrc/gemm_big.hip)
FUSION_NONE, FUSION_REPLACE, FUSION_LINEAR = 0, 1, 2

_i64, _i32, _f32, _vp, _sz = C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_size_t


class Stream32(C.Structure):
    """``vface_stream32`` of the header: the optional fp32 residual-stream operands of a GEMM-family call."""
    _fields_ = [("residual32", _vp), ("ldr32", _i64), ("out32", _vp), ("ldo32", _i64),
                ("in_scale_shift", _vp), ("ld_scale_shift", _i64), ("in_silu", _i32)]


_s32p = C.POINTER(Stream32)

# name -> (restype, argtypes); mirrors include/vface_hip.h one to one
SIGNATURES = {
    "vface_abi_version": (C.c_int, []),
    "vface_error_string": (C.c_char_p, [_i32]),
    "vface_gemm_variants_built": (C.c_int, []),
    "vface_gemm": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp,
                             _i64, _vp, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _s32p]),
    "vface_conv3x3": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp,
                                _i64, _vp, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _s32p]),
    "vface_splitk_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "vface_conv_uses_patch_kernel": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "vface_conv3x3_plus_1x1": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp, _i32,
                                         _vp, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _s32p]),
    "vface_upsample2x_conv3x3_phase": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _i32,
                                                 _vp, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _s32p]),
    "vface_groupnorm_finalize_cols": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _f32, _vp, _vp]),
    "vface_attention": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i32,
                                  _i32, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _vp]),
    "vface_attention_shared_scores_supported": (C.c_int, [_i32, _i32]),
    "vface_layernorm": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _i32, _i32, _vp]),
    "vface_groupnorm_partial_floats": (C.c_int, [_i32, _i32, _i32, _i32]),
    "vface_groupnorm_stats": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _i32, _vp]),
    "vface_groupnorm_coeffs_from_cols": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "vface_groupnorm_apply": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vface_flow_warp": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _f32,
                                  _f32, _i32, _vp, _vp, _i32, _vp]),
    "vface_flow_to_latent": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "vface_im2col": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "vface_channel_stats_partial_floats": (_i64, [_i32, _i32, _i32]),
    "vface_channel_stats": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _vp]),
    "vface_channel_norm_act": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "vface_gru_gate": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
    "vface_gru_update": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
    "vface_avgpool2_f32": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "vface_corr_lookup": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _vp, _i64, _i64, _i32, _vp]),
    "vface_flow_update": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp]),
    "vface_convex_upsample": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "vface_frame_to_u8": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "vface_resample_u8": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "vface_perspective_paste": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vface_frame_normalise_resize": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "vface_rgb_to_yuv420": (C.c_int, [_vp, _i32, _i32, _vp, _i64, _i32, _vp]),
    "vface_jpeg_coefficients": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "vface_jpeg_entropy_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "vface_jpeg_entropy": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _sz, _vp]),
    "vface_png_filter": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "vface_png_deflate_bound": (_i64, [_i32, _i32, _i32]),
    "vface_png_deflate_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "vface_png_deflate": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vface_gif_histogram": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "vface_gif_boxes": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    "vface_gif_palette": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vface_gif_map": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vface_gif_lzw_bound": (_i64, [_i64, _i32]),
    "vface_gif_lzw_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vface_gif_lzw": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _sz, _vp]),
    "vface_png_inflate": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "vface_png_unfilter": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vface_png_inflate_parallel_workspace_bytes": (_sz, [_i32, _i64, _i64, _i32]),
    "vface_png_inflate_parallel": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _sz, _vp, _vp]),
    "vface_yuv420_to_rgb": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "vface_jpeg_scan_index": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vface_jpeg_decode_entropy": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "vface_jpeg_decode_entropy_parallel_workspace_bytes": (_sz, [_i32]),
    "vface_jpeg_decode_entropy_parallel": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _vp, _sz, _vp, _vp]),
    "vface_jpeg_planes": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _vp, _i64, _vp]),
    "vface_quad_crop": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "vface_dataset_tensors": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "vface_source_tensors": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp,
                                       _i32, _i32, _vp]),
    "vface_parse_prefilter": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _vp]),
    "vface_maxpool3x3s2": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "vface_channel_gate": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "vface_pooled_linear": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "vface_upsample_argmax_u8": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp]),
    "vface_clip_patches": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp]),
    "vface_clip_embed": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "vface_act": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "vface_cond_mix": (C.c_int, [_vp, _i32, _f32, _vp, _i32, _f32, _vp, _i32, _f32, _f32, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp]),
    "vface_id_prep": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp]),
    "vface_prelu": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "vface_se_gate_add": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _i32,
                                    _vp]),
    "vface_l2norm_rows": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "vface_ffn_fused_supported": (C.c_int, [_i64, _i32]),
    "vface_ffn_fused": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp]),
    "vface_attn_out_ffn_fused": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _i64, _vp,
                                           _i64, _i32, _i32, _i32, _vp]),
    "vface_attn_out_ffn_proj_fused": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp,
                                                _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp]),
    "vface_linear_small_supported": (C.c_int, [_i32, _i32, _i32]),
    "vface_linear_small": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vface_gn_silu_conv3x3_small": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vface_st_front_supported": (C.c_int, [_i64, _i32, _i32]),
    "vface_st_front": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32,
                                 _i32, _i32, _i32, _vp]),
    "vface_temporal_gauss": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "vface_adain_workspace_bytes": (_sz, [_i64, _i32]),
    "vface_adain_fusion": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _sz, _i32, _vp]),
    "vface_temporal_gauss_halo": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32,
                                            _i32, _i32, _vp]),
    "vface_adain_rows_workspace_bytes": (_sz, [_i64, _i32]),
    "vface_adain_rows": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _sz, _i32, _vp]),
    "vface_adain_reduce_scale": (C.c_int, [_vp, _i64, _i32, _vp, _sz, _vp, _i64, _i64, _i32, _vp]),
    "vface_timestep_embedding": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "vface_silu": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "vface_softmax_rows": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _f32, _i32, _vp]),
    "vface_vae_sample": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, _f32, _vp]),
    "vface_cast_f32": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "vface_pack_unet_input": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vface_nchw_to_nhwc": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vface_nhwc_to_nchw_f32": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _vp]),
    "vface_ddim_step": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _f32,
                                  _vp, _i32, _vp]),
    "vface_copy2d": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
}

_lib = None


class VFaceHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the library and bind every symbol of the header; raises if it is absent (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VFaceHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  The VFace path has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.vface_abi_version() != 8:
        raise VFaceHipError("libvface_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = load().vface_error_string(rc).decode()
        raise VFaceHipError(f"{what}: {msg} (code {rc})")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float16:
        return F16
    if dt == torch.bfloat16:
        return BF16
    raise VFaceHipError(f"unsupported dtype {dt}: the HIP path computes in fp16 or bf16")


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise VFaceHipError("tensor is not on the GPU: the VFace hot path has no CPU fallback")
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _s32(residual32: Optional[torch.Tensor], out32: Optional[torch.Tensor], gn_ab: Optional[torch.Tensor] = None,
         gn_silu: bool = False):
    """The ``vface_stream32`` argument: fp32 residual operand and / or fp32 copy of the output (2-D views, unit column
    stride), and for convolutions the fused input normalisation ``gn_ab`` ``[nimg, C, 2]`` fp32; None when nothing is given."""
    if residual32 is None and out32 is None and gn_ab is None:
        return None
    for t in (residual32, out32):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1):
            raise VFaceHipError("fp32 residual-stream tensors must be 2-D fp32 views with unit column stride")
    if gn_ab is not None and (gn_ab.dtype != torch.float32 or gn_ab.dim() != 3 or gn_ab.shape[2] != 2 or not gn_ab.is_contiguous()):
        raise VFaceHipError("gn_ab must be a contiguous fp32 [nimg, C, 2] tensor (groupnorm_coeffs_from_cols)")
    return C.byref(Stream32(_p(residual32), residual32.stride(0) if residual32 is not None else 0,
                            _p(out32), out32.stride(0) if out32 is not None else 0,
                            _p(gn_ab), gn_ab.shape[1] if gn_ab is not None else 0, int(gn_silu)))


_zeros = {}


def zeros_page(device) -> torch.Tensor:
    """A 256-byte zero page the implicit-GEMM kernels read for padding taps / tile tails."""
    key = str(device)
    if key not in _zeros:
        _zeros[key] = torch.zeros(256, dtype=torch.uint8, device=device)
    return _zeros[key]


_splitk_ws = {}
_ws_domain = 0


class workspace_domain:
    """``with hip.workspace_domain(k):`` -- launches inside take split-K scratch number k.  Launches on ONE stream use a scratch in
    order; a caller that runs two launch sequences on two streams at once (the engine's two half-batches) gives each its own."""

    def __init__(self, k: int):
        self.k = int(k)

    def __enter__(self):
        global _ws_domain
        self.prev, _ws_domain = _ws_domain, self.k
        return self

    def __exit__(self, *exc):
        global _ws_domain
        _ws_domain = self.prev
        return False


def splitk_workspace(device, M: int, N: int, K: int, flags: int = 0, rows_per_sample: int = 1):
    """Device scratch for a split-K launch of this shape (grown on demand, one per device and workspace domain; launches on
    one stream use it in order).  Returns (tensor | None, bytes)."""
    need = load().vface_splitk_workspace_bytes(M, N, K, flags, rows_per_sample)
    if need <= 0:
        return None, 0
    key = str(device) if _ws_domain == 0 else f"{device}#{_ws_domain}"
    ws = _splitk_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _splitk_ws[key] = ws
    return ws, ws.numel()


# ---------------------------------------------------------------------------------------------- wrappers
# What a caller can check before it launches anything (csrc/dispatch.cpp ``validate``: ``K & 7``, ``lda & 7``, ``ldw & 7`` are
# VFACE_ERR_ALIGN and an operand view of 4 GiB - 16 bytes or more is VFACE_ERR_SHAPE; ``vface_softmax_rows``: ``N & 3`` and
# ``N > 16384``).  A GEMM whose K is a row of softmax output needs both rules of its length: a multiple of 8, at most 16384.
GEMM_K_MULTIPLE = 8
SOFTMAX_MAX_COLS = 16384
OPERAND_BYTES_LIMIT = 0xFFFFFFF0


def gemm(a: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, *, M: int, N: int, K: int, lda: int, ldc: int,
         ldw: Optional[int] = None, bias=None, rowbias=None, rows_per_sample: int = 1, residual=None, ldr: int = 0,
         a2=None, lda2: int = 0, k1: int = 0, a2_row_mod: int = 0, flags: int = 0, colstats=None, split_k: bool = True,
         residual32=None, out32=None):
    """out[M, :N] = a[M, :K] @ wt[:N, :K]^T (+ epilogue).  Tensors are device buffers; M/N/K/ld* describe the view.
    ``residual32`` / ``out32``: the fp32 residual stream (``vface_stream32``); ``out`` may be None with ``out32``."""
    lib = load()
    ws, ws_bytes = splitk_workspace(a.device, M, N, K, flags, rows_per_sample) if split_k else (None, 0)
    rc = lib.vface_gemm(_p(a), lda, _p(a2), lda2, k1, a2_row_mod, _p(wt), ldw if ldw is not None else K, M, N, K,
                        _p(bias), _p(rowbias), rows_per_sample, rowbias.stride(0) if rowbias is not None else 0,
                        _p(residual), ldr, _p(out), ldc, _p(zeros_page(a.device)), flags, dtype_code(a.dtype),
                        _p(colstats), colstats.stride(0) // 2 if colstats is not None else 0, _p(ws), ws_bytes, _stream(),
                        _s32(residual32, out32))
    _check(rc, "vface_gemm")


def conv3x3(x: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, *, nimg: int, H: int, W: int, cin: int, cout: int,
            ldx: int, ldy: int, stride: int = 1, upsample: bool = False, bias=None, rowbias=None, residual=None,
            ldr: int = 0, flags: int = 0, colstats=None, split_k: bool = True, residual32=None, out32=None, gn_ab=None,
            gn_silu: bool = False):
    """``gn_ab`` (+ ``gn_silu``): GroupNorm-apply (+ SiLU) of the INPUT fused into the patch-staged kernel's operand path."""
    lib = load()
    vh, vw = (2 * H, 2 * W) if upsample else (H, W)
    M = nimg * ((vh - 1) // stride + 1) * ((vw - 1) // stride + 1)
    ws, ws_bytes = splitk_workspace(x.device, M, cout, 9 * cin, flags, M // nimg) if split_k else (None, 0)
    rc = lib.vface_conv3x3(_p(x), ldx, nimg, H, W, cin, _p(wt), 9 * cin, cout, stride, int(upsample), _p(bias),
                           _p(rowbias), rowbias.stride(0) if rowbias is not None else 0, _p(residual), ldr, _p(out),
                           ldy, _p(zeros_page(x.device)), flags, dtype_code(x.dtype), _p(colstats),
                           colstats.stride(0) // 2 if colstats is not None else 0, _p(ws), ws_bytes, _stream(),
                           _s32(residual32, out32, gn_ab, gn_silu))
    _check(rc, "vface_conv3x3")


def conv_uses_patch_kernel(H: int, W: int, cin: int, cout: int, window: int = 3, stride: int = 1, upsample: bool = False,
                           flags: int = 0) -> int:
    """Which kernel a convolution launch of this geometry runs: 1 = conv.hip's patch-staged kernel, 2 = its 8x8 form (four
    images per workgroup + split-K reduce), 0 = gemm.hip's implicit GEMM."""
    return int(load().vface_conv_uses_patch_kernel(H, W, cin, cout, window, stride, int(upsample), flags))


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, B: int, heads: int, n: int,
              nk: int, dh: int, ldq: int, ldk: int, ldv: int, bsq: int, bsk: int, bsv: int, ldo: int, bso: int,
              scale: float, qk_map=None, v_map=None, variant: int = 0, v_sets: int = 1, set_stride: int = 0,
              v_sets_live: int = 0):
    """``v_sets > 1``: B q/k samples, output sample ``b + g*set_stride`` uses v of that sample (through ``v_map``)
    with the probabilities of q/k sample b, computed once (the "replace" injection).  ``v_sets_live`` (2 of 3): only the first
    sets exist in the batch; their outputs are those of the full call bit for bit."""
    lib = load()
    rc = lib.vface_attention(_p(q), _p(k), _p(v), ldq, ldk, ldv, bsq, bsk, bsv, _p(qk_map), _p(v_map), _p(out), ldo,
                             bso, B, heads, n, nk, dh, scale, dtype_code(out.dtype) | (variant << 8),
                             v_sets | ((v_sets_live if v_sets_live != v_sets else 0) << 8), set_stride, _stream())
    _check(rc, "vface_attention")


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, *, M: int, C_: int,
              ldx: int, ldy: int, eps: float = 1e-5):
    rc = load().vface_layernorm(_p(x), ldx, _p(gamma), _p(beta), _p(out), ldy, M, C_, eps,
                                int(x.dtype == torch.float32), dtype_code(out.dtype), _stream())
    _check(rc, "vface_layernorm")


def groupnorm_stats(x: torch.Tensor, *, nimg: int, hw: int, C_: int, ldx: int, groups: int = 32, eps: float = 1e-5):
    lib = load()
    nf = lib.vface_groupnorm_partial_floats(nimg, hw, C_, groups)
    partial = torch.empty(nf, dtype=torch.float32, device=x.device)
    stats = torch.empty(nimg, groups, 2, dtype=torch.float32, device=x.device)
    in32 = x.dtype == torch.float32
    rc = lib.vface_groupnorm_stats(_p(x), ldx, nimg, hw, C_, groups, eps, _p(partial), _p(stats), int(in32),
                                   F16 if in32 else dtype_code(x.dtype), _stream())
    _check(rc, "vface_groupnorm_stats")
    return stats


def groupnorm_stats_from_cols(colstats: torch.Tensor, *, nimg: int, hw: int, C_: int, groups: int = 32, eps: float = 1e-5):
    """colstats: [nimg*hw/64, C(view), 2] fp32 view (row stride = 2 * ld)."""
    stats = torch.empty(nimg, groups, 2, dtype=torch.float32, device=colstats.device)
    rc = load().vface_groupnorm_finalize_cols(_p(colstats), colstats.stride(0) // 2, nimg, hw, C_, groups, eps, _p(stats),
                                              _stream())
    _check(rc, "vface_groupnorm_finalize_cols")
    return stats


def groupnorm_coeffs_from_cols(colstats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, nimg: int, hw: int, C_: int,
                               groups: int = 32, eps: float = 1e-5) -> torch.Tensor:
    """Per-(image, channel) scale / shift (a, b) of GroupNorm from producer-side column statistics: fp32 [nimg, C, 2]."""
    ab = torch.empty(nimg, C_, 2, dtype=torch.float32, device=colstats.device)
    rc = load().vface_groupnorm_coeffs_from_cols(_p(colstats), colstats.stride(0) // 2, nimg, hw, C_, groups, eps, _p(gamma),
                                                 _p(beta), _p(ab), _stream())
    _check(rc, "vface_groupnorm_coeffs_from_cols")
    return ab


def groupnorm_apply(x: torch.Tensor, stats: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor,
                    *, nimg: int, hw: int, C_: int, ldx: int, ldy: int, groups: int = 32, silu: bool = False):
    rc = load().vface_groupnorm_apply(_p(x), ldx, _p(stats), _p(gamma), _p(beta), _p(out), ldy, nimg, hw, C_, groups,
                                      int(silu), int(x.dtype == torch.float32), dtype_code(out.dtype), _stream())
    _check(rc, "vface_groupnorm_apply")


def flow_warp(src: torch.Tensor, dst: torch.Tensor, flow: Optional[torch.Tensor], *, F: int, h: int, w: int, C_: int,
              ld_src: int, fs_src: int, ld_dst: int, fs_dst: int, alpha: float, prev=None, ld_prev: int = 0,
              flow_prev=None, cuda_recip_div: bool = False, dbg_x0=None, dbg_y0=None):
    # python-double (1 - alpha) rounded to fp32, as the reference's scalar * fp32-tensor product sees it
    rc = load().vface_flow_warp(_p(src), ld_src, fs_src, _p(prev), ld_prev, _p(flow), _p(flow_prev), _p(dst), ld_dst,
                                fs_dst, F, h, w, C_, float(alpha), float(1.0 - alpha), int(cuda_recip_div),
                                _p(dbg_x0), _p(dbg_y0), dtype_code(src.dtype), _stream())
    _check(rc, "vface_flow_warp")


def flow_to_latent(flow_px: torch.Tensor, factor: int = 8) -> torch.Tensor:
    """[P, 2, H, W] fp32 pixel-resolution flow -> [P, 2, H/factor, W/factor] latent-resolution flow (area mean / factor)."""
    if flow_px.dim() != 4 or flow_px.shape[1] != 2:
        raise VFaceHipError(f"flow must be [pairs, 2, H, W]; got {tuple(flow_px.shape)}")
    f = flow_px.to(dtype=torch.float32).contiguous()
    P, _, H, W = f.shape
    out = torch.empty(P, 2, H // factor, W // factor, dtype=torch.float32, device=f.device)
    rc = load().vface_flow_to_latent(_p(f), _p(out), P, H, W, factor, _stream())
    _check(rc, "vface_flow_to_latent")
    return out


# ---- glue of the RAFT-shaped flow producer (csrc/raft.hip; include/vface_hip.h "optical-flow producer") ----
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3


def im2col(x: torch.Tensor, out: torch.Tensor, *, nimg: int, H: int, W: int, C_: int, kh: int, kw: int, stride: int = 1,
           pad_y: int = 0, pad_x: int = 0, ldx: Optional[int] = None):
    rc = load().vface_im2col(_p(x), ldx if ldx is not None else x.stride(0), nimg, H, W, C_, kh, kw, stride, pad_y, pad_x, _p(out),
                             out.stride(0), dtype_code(x.dtype), _stream())
    _check(rc, "vface_im2col")


def channel_stats(x: torch.Tensor, *, nimg: int, hw: int, C_: int, ldx: Optional[int] = None, eps: float = 1e-5) -> torch.Tensor:
    lib = load()
    partial = torch.empty(int(lib.vface_channel_stats_partial_floats(nimg, hw, C_)), dtype=torch.float32, device=x.device)
    stats = torch.empty(nimg, C_, 2, dtype=torch.float32, device=x.device)
    rc = lib.vface_channel_stats(_p(x), ldx if ldx is not None else x.stride(0), nimg, hw, C_, eps, _p(partial), _p(stats),
                                 dtype_code(x.dtype), _stream())
    _check(rc, "vface_channel_stats")
    return stats


def channel_norm_act(x: torch.Tensor, y: Optional[torch.Tensor], *, M: int, hw: int, C_: int, act: int, stats=None, residual=None,
                     y32=None, ldx: Optional[int] = None, ldy: Optional[int] = None, ldr: Optional[int] = None):
    rc = load().vface_channel_norm_act(_p(x), ldx if ldx is not None else x.stride(0), _p(stats), _p(residual),
                                       (ldr if ldr is not None else residual.stride(0)) if residual is not None else 0, _p(y),
                                       (ldy if ldy is not None else y.stride(0)) if y is not None else 0, _p(y32),
                                       y32.stride(0) if y32 is not None else 0, M, hw, C_, act, dtype_code(x.dtype), _stream())
    _check(rc, "vface_channel_norm_act")


def gru_gate(zr: torch.Tensor, h32: torch.Tensor, z: torch.Tensor, rh: torch.Tensor, *, M: int, hidden: int, ldrh: int):
    rc = load().vface_gru_gate(_p(zr), zr.stride(0), _p(h32), _p(z), z.stride(0), _p(rh), ldrh, M, hidden, dtype_code(zr.dtype), _stream())
    _check(rc, "vface_gru_gate")


def gru_update(q: torch.Tensor, z: torch.Tensor, h32: torch.Tensor, h16a, lda: int, h16b, ldb: int, *, M: int, hidden: int):
    rc = load().vface_gru_update(_p(q), q.stride(0), _p(z), z.stride(0), _p(h32), _p(h16a), lda, _p(h16b), ldb, M, hidden,
                                 dtype_code(q.dtype), _stream())
    _check(rc, "vface_gru_update")


def avgpool2_f32(x: torch.Tensor, y: torch.Tensor, *, R: int, h: int, w: int):
    _check(load().vface_avgpool2_f32(_p(x), _p(y), R, h, w, _stream()), "vface_avgpool2_f32")


def corr_lookup(vols, flow32: torch.Tensor, out: torch.Tensor, *, h: int, w: int, scale: float):
    n = len(vols)
    ptrs = (C.c_void_p * n)(*[_p(v) for v in vols])
    hs = (C.c_int * n)(*[int(v.shape[-2]) for v in vols])
    ws = (C.c_int * n)(*[int(v.shape[-1]) for v in vols])
    rc = load().vface_corr_lookup(C.cast(ptrs, C.c_void_p), C.cast(hs, C.c_void_p), C.cast(ws, C.c_void_p), n, _p(flow32), h, w,
                                  scale, _p(out), out.stride(0), flow32.shape[0], dtype_code(out.dtype), _stream())
    _check(rc, "vface_corr_lookup")


def flow_update(flow32: torch.Tensor, delta32, copies, *, dtype: torch.dtype):
    """``copies``: up to three (tensor view whose first two columns receive the 16-bit flow, row stride) pairs."""
    c = list(copies) + [(None, 0)] * (3 - len(copies))
    rc = load().vface_flow_update(_p(flow32), _p(delta32), delta32.stride(0) if delta32 is not None else 0, _p(c[0][0]), c[0][1],
                                  _p(c[1][0]), c[1][1], _p(c[2][0]), c[2][1], flow32.shape[0], dtype_code(dtype), _stream())
    _check(rc, "vface_flow_update")


def convex_upsample(mask32: torch.Tensor, flow32: torch.Tensor, *, B: int, h: int, w: int, mult: float = 0.25) -> torch.Tensor:
    out = torch.empty(B, 2, 8 * h, 8 * w, dtype=torch.float32, device=mask32.device)
    rc = load().vface_convex_upsample(_p(mask32), mask32.stride(0), _p(flow32), _p(out), B, h, w, mult, _stream())
    _check(rc, "vface_convex_upsample")
    return out


def frame_to_u8(x: torch.Tensor, half_arithmetic: bool = False) -> torch.Tensor:
    """Decoded frames [F, 3, H, W] in [-1, 1] (fp16 / bf16 / fp32) -> uint8 [F, H, W, 3]: clamp((x + 1) / 2, 0, 1) * 255, truncated.
    The arithmetic is **fp32** whatever the input type -- the reference's ``--precision full`` run.  ``half_arithmetic=True`` (fp16
    input only) rounds every operation to float16 instead, which is what the reference's default ``--precision autocast`` run
    computes on the float16 tensor ``decode_first_stage`` returns (:597-608); the two can differ by one in a pixel."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise VFaceHipError(f"frame_to_u8: frames must be [F, 3, H, W]; got {tuple(x.shape)}")
    x = x.contiguous()
    if half_arithmetic and x.dtype != torch.float16:
        raise VFaceHipError("frame_to_u8(half_arithmetic=True) takes float16 frames (the autocast path's decode output)")
    kind = 3 if half_arithmetic else (2 if x.dtype == torch.float32 else dtype_code(x.dtype))
    F_, _, H, W = x.shape
    out = torch.empty(F_, H, W, 3, dtype=torch.uint8, device=x.device)
    _check(load().vface_frame_to_u8(_p(x), _p(out), F_, H, W, kind, _stream()), "vface_frame_to_u8")
    return out


def resample_u8(src: torch.Tensor, out_n: int, axis: int, bounds: torch.Tensor, kk: torch.Tensor) -> torch.Tensor:
    """One pass of Pillow's 8-bit bilinear resampling over uint8 [F, H, W, 3] frames: axis 0 along x (W -> out_n), axis 1 along y."""
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or not src.is_contiguous():
        raise VFaceHipError("resample_u8: frames must be contiguous uint8 [F, H, W, 3]")
    if bounds.dtype != torch.int32 or kk.dtype != torch.int32 or tuple(bounds.shape) != (out_n, 2) or kk.shape[0] != out_n:
        raise VFaceHipError("resample_u8: bounds [out_n, 2] / kk [out_n, ksize] must be int32 tables for this output size")
    F_, H, W, _ = src.shape
    if axis == 0:
        dst = torch.empty(F_, H, out_n, 3, dtype=torch.uint8, device=src.device)
        in_n, lines = W, H
    else:
        dst = torch.empty(F_, out_n, W, 3, dtype=torch.uint8, device=src.device)
        in_n, lines = H, W
    rc = load().vface_resample_u8(_p(src), _p(dst), F_, in_n, out_n, lines, axis, _p(bounds), _p(kk), kk.shape[1], _stream())
    _check(rc, "vface_resample_u8")
    return dst


def perspective_paste(crop: torch.Tensor, frame: torch.Tensor, coeffs) -> torch.Tensor:
    """Paste uint8 crops [F, h, w, 3] into uint8 frames [F, H, W, 3] IN PLACE through the eight PIL perspective coefficients per
    frame (``coeffs``: a float64 device tensor [F, 8], or eight host floats when F == 1)."""
    for t in (crop, frame):
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or not t.is_contiguous():
            raise VFaceHipError("perspective_paste: crops and frames must be contiguous uint8 [F, H, W, 3]")
    F_, sh, sw, _ = crop.shape
    if frame.shape[0] != F_:
        raise VFaceHipError("perspective_paste: one crop per frame")
    dev_c, host_c = None, None
    if isinstance(coeffs, torch.Tensor) and coeffs.is_cuda:
        if coeffs.dtype != torch.float64 or tuple(coeffs.shape) != (F_, 8) or not coeffs.is_contiguous():
            raise VFaceHipError("perspective_paste: device coefficients must be contiguous float64 [F, 8]")
        dev_c = coeffs
    else:
        vals = [float(v) for v in (coeffs.reshape(-1).tolist() if hasattr(coeffs, "reshape") else coeffs)]
        if len(vals) != 8 or F_ != 1:
            raise VFaceHipError("perspective_paste: host coefficients are eight numbers for a single frame")
        host_c = (C.c_double * 8)(*vals)
    rc = load().vface_perspective_paste(_p(crop), sw, sh, _p(frame), frame.shape[2], frame.shape[1], F_, _p(dev_c),
                                        C.cast(host_c, C.c_void_p) if host_c is not None else None, _stream())
    _check(rc, "vface_perspective_paste")
    return frame


def frame_normalise_resize(frame: torch.Tensor, OH: int, OW: int) -> torch.Tensor:
    """uint8 frames [F, H, W, 3] -> fp32 [F, 3, OH, OW] in [-1, 1]: ToTensor + Normalize(0.5, 0.5) + bilinear Resize (no antialias)."""
    if frame.dtype != torch.uint8 or frame.dim() != 4 or frame.shape[3] != 3 or not frame.is_contiguous():
        raise VFaceHipError("frame_normalise_resize: frames must be contiguous uint8 [F, H, W, 3]")
    F_, H, W, _ = frame.shape
    out = torch.empty(F_, 3, OH, OW, dtype=torch.float32, device=frame.device)
    _check(load().vface_frame_normalise_resize(_p(frame), W, H, _p(out), OW, OH, F_, _stream()), "vface_frame_normalise_resize")
    return out


def i420_frame_bytes(W: int, H: int) -> int:
    """Bytes of one I420 frame: Y [H][W] + Cb and Cr [(H + 1) / 2][(W + 1) / 2]."""
    return W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)


def rgb_to_yuv420(frames_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 frames [F, H, W, 3] (what ``PasteBack.paste`` returns) -> uint8 [F, frame_bytes]: per frame the I420 planes Y [H][W],
    Cb [ch][cw], Cr [ch][cw] -- BT.709, limited range, chroma centre-sited; the integer arithmetic of ``tests/mux_model.py``, bit
    for bit (csrc/mux.hip).  ``out``: a uint8 [F, frame_bytes] view with unit column stride and a row stride of at least
    frame_bytes (frames inside a larger buffer); the bytes between frames are not written."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise VFaceHipError("rgb_to_yuv420: frames must be contiguous uint8 [F, H, W, 3]")
    F_, H, W, _ = frames_u8.shape
    if min(F_, H, W) <= 0:
        raise VFaceHipError("rgb_to_yuv420: F, H and W must be positive")
    n = i420_frame_bytes(W, H)
    if out is None:
        out = torch.empty(F_, n, dtype=torch.uint8, device=frames_u8.device)
    elif (out.dtype != torch.uint8 or tuple(out.shape) != (F_, n) or out.stride(1) != 1 or (F_ > 1 and out.stride(0) < n)
          or out.device != frames_u8.device):
        raise VFaceHipError(f"rgb_to_yuv420: out must be a uint8 {[F_, n]} view on the frames' device, unit column stride, "
                            f"row stride >= {n}")
    stride = out.stride(0) if F_ > 1 else max(out.stride(0), n)
    _check(load().vface_rgb_to_yuv420(_p(frames_u8), W, H, _p(out), stride, F_, _stream()), "vface_rgb_to_yuv420")
    return out


JPEG_MCU_COEFS = 6 * 64            # int16 elements of one 16 x 16 MCU: Y00 Y01 Y10 Y11 Cb Cr
JPEG_BLOCK_BYTES_BOUND = 416       # worst case of one coded block: 64 x (16 + 10) bits, doubled for the stuffing (csrc/mjpeg.hip)
_jpeg_ws = {}


def jpeg_mcu_grid(W: int, H: int) -> Tuple[int, int]:
    """(mcu_rows, mcu_cols) of a W x H frame: 16 x 16 pixels per MCU, the last column and row replicated."""
    return (int(H) + 15) // 16, (int(W) + 15) // 16


def jpeg_scan_bytes_bound(mcus: int, restart: int) -> int:
    """Bytes that always hold one frame's scan (``vface_jpeg_entropy`` in the header): every block at its worst, RST markers."""
    nint = -(-int(mcus) // int(restart))
    return nint * min(int(restart), int(mcus)) * 6 * JPEG_BLOCK_BYTES_BOUND + 2 * (nint - 1)


def jpeg_coefficients(frames_u8: torch.Tensor, qluma: torch.Tensor, qchroma: torch.Tensor,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 frames [F, H, W, 3] -> the quantised DCT coefficients of a baseline 4:2:0 JPEG, int16 [F, mcu_rows, mcu_cols, 6, 64]:
    the blocks Y00 Y01 Y10 Y11 Cb Cr of every 16 x 16 MCU, zigzag order; a frame is extended to whole MCUs by replicating its last
    column and row.  The colour matrix is **full-range BT.601 (JFIF)**, what every MJPEG decoder assumes -- not the BT.709 ``tv``
    range of ``rgb_to_yuv420``.  ``qluma``, ``qchroma``: device uint8 [64], row-major, 1..255 (``scripts/mjpeg.quant_tables``).
    The integer arithmetic of ``tests/jpeg_model.py``, bit for bit (csrc/mjpeg.hip).  ``out``: an int16 view of that shape whose
    frames are contiguous, frame stride at least one frame; the elements between frames are not written."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise VFaceHipError("jpeg_coefficients: frames must be contiguous uint8 [F, H, W, 3]")
    F_, H, W, _ = frames_u8.shape
    if min(F_, H, W) <= 0:
        raise VFaceHipError("jpeg_coefficients: F, H and W must be positive")
    for q in (qluma, qchroma):
        if q.dtype != torch.uint8 or tuple(q.shape) != (64,) or not q.is_contiguous() or q.device != frames_u8.device:
            raise VFaceHipError("jpeg_coefficients: a quantisation table is a contiguous uint8 [64] tensor on the frames' device")
    mr, mc = jpeg_mcu_grid(W, H)
    shape, n = (F_, mr, mc, 6, 64), mr * mc * JPEG_MCU_COEFS
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=frames_u8.device)
    elif (out.dtype != torch.int16 or tuple(out.shape) != shape or not out[0].is_contiguous() or (F_ > 1 and out.stride(0) < n)
          or out.device != frames_u8.device):
        raise VFaceHipError(f"jpeg_coefficients: out must be an int16 {list(shape)} view on the frames' device, frames contiguous, "
                            f"frame stride >= {n}")
    stride = out.stride(0) if F_ > 1 else max(out.stride(0), n)
    _check(load().vface_jpeg_coefficients(_p(frames_u8), W, H, F_, _p(qluma), _p(qchroma), _p(out), stride, _stream()),
           "vface_jpeg_coefficients")
    return out


def jpeg_entropy(coef: torch.Tensor, restart: int, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Coefficient frames, device int16 [F, mcu_rows, mcu_cols, 6, 64] (or [F, mcus, 6, 64]; what ``jpeg_coefficients`` returns, a
    frame stride is fine) -> ``(out, lengths)``: the entropy-coded scans of the frames packed back to back in the uint8 buffer
    ``out`` and int32 ``lengths`` [F], so the host copies ``out[:lengths.sum()]`` and nothing else.  Baseline Huffman coding, the
    Annex-K tables, restart intervals of ``restart`` MCUs with RSTm between them, no EOI (csrc/mjpeg.hip; equal to
    ``tests/jpeg_model.scan_bytes`` byte for byte).  ``out``: a contiguous uint8 buffer; by default one of the worst-case size
    (``jpeg_scan_bytes_bound``).  Bytes that a smaller ``out`` cannot hold are dropped, and the caller sees it from the lengths."""
    if (not isinstance(coef, torch.Tensor) or coef.dtype != torch.int16 or coef.dim() not in (4, 5) or tuple(coef.shape[-2:]) != (6, 64)
            or not coef[0].is_contiguous()):
        raise VFaceHipError("jpeg_entropy: coefficients must be int16 [F, mcu_rows, mcu_cols, 6, 64] with contiguous frames")
    F_, mcus, restart = coef.shape[0], coef[0].numel() // JPEG_MCU_COEFS, int(restart)
    if min(F_, mcus) <= 0 or not 1 <= restart <= 65535:
        raise VFaceHipError(f"jpeg_entropy: F and the MCUs per frame must be positive, restart in 1..65535; got {F_}, {mcus}, {restart}")
    n = mcus * JPEG_MCU_COEFS
    if F_ > 1 and coef.stride(0) < n:
        raise VFaceHipError(f"jpeg_entropy: frame stride >= {n}")
    if out is None:
        out = torch.empty(F_ * jpeg_scan_bytes_bound(mcus, restart), dtype=torch.uint8, device=coef.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != coef.device or out.numel() == 0:
        raise VFaceHipError("jpeg_entropy: out must be a contiguous uint8 buffer on the coefficients' device")
    lib = load()
    need = int(lib.vface_jpeg_entropy_workspace_bytes(mcus, F_, restart))
    ws = _jpeg_ws.get(str(coef.device))
    if ws is None or ws.numel() < need:
        ws = _jpeg_ws[str(coef.device)] = torch.empty(need, dtype=torch.uint8, device=coef.device)
    lengths = torch.empty(F_, dtype=torch.int32, device=coef.device)
    stride = coef.stride(0) if F_ > 1 else max(coef.stride(0), n)
    _check(lib.vface_jpeg_entropy(_p(coef), stride, mcus, F_, restart, _p(out), out.numel(), _p(lengths), _p(ws), ws.numel(),
                                  _stream()), "vface_jpeg_entropy")
    return out, lengths


# ---- PNG frames out (:636; csrc/png.hip)
PNG_STRIPE_ROWS = 16               # rows of a frame that make one independent deflate block: tools/bench_png.py's sweep over 4, 8, 16, 32
                                   # (profiles/r11_a_*): the fastest at 512 x 512, within 5 % of 8 at 1920 x 1080, smaller files than either
PNG_FILTER_GRID_CAP = 2048         # kPngFilterGridCap: workgroups of PNG_FILTER_ROWS_PER_GROUP rows before the grid loops
PNG_FILTER_ROWS_PER_GROUP = 4
PNG_DEFLATE_GRID_CAP = 4096        # kPngDeflateGridCap: workgroups, one (frame, stripe) each, before the grid loops
_png_ws = {}


def png_deflate_bound(row_bytes: int, rows: int, stripe_rows: int = PNG_STRIPE_ROWS) -> int:
    """Bytes that always hold the deflate body of ``rows`` rows of ``row_bytes`` bytes: every stripe as stored blocks of at most
    65535 bytes (5 bytes of header each) and the final ``03 00``.  Exact for incompressible rows: a stripe whose dynamic block
    would not be smaller is stored."""
    return int(load().vface_png_deflate_bound(int(row_bytes), int(rows), int(stripe_rows)))


def png_filter(frames_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 device frames [F, H, W, 3] -> uint8 [F, H, 1 + 3 W]: every row's PNG filter byte and filtered bytes (:636).  A row takes
    the type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; bpp 3; zeros above row 0) whose filtered bytes, read as signed, have the
    smallest sum of absolute values, a tie the lowest type; ``tests/png_model.filter_rows`` bit for bit (csrc/png.hip)."""
    if (not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4
            or frames_u8.shape[-1] != 3 or not frames_u8.is_contiguous()):
        raise VFaceHipError("png_filter: frames must be contiguous uint8 [F, H, W, 3] on the GPU")
    F_, H, W, _ = frames_u8.shape
    if min(F_, H, W) <= 0:
        raise VFaceHipError("png_filter: F, H and W must be positive")
    shape = (F_, H, 1 + 3 * W)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames_u8.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != frames_u8.device or not out.is_contiguous():
        raise VFaceHipError(f"png_filter: out must be a contiguous uint8 {list(shape)} tensor on the frames' device")
    _check(load().vface_png_filter(_p(frames_u8), W, H, F_, _p(out), _stream()), "vface_png_filter")
    return out


def png_deflate(rows: torch.Tensor, stripe_rows: int = PNG_STRIPE_ROWS, out: Optional[torch.Tensor] = None):
    """Row buffers of ANY bytes, device uint8 [F, H, row_bytes] -> ``(out, meta, offsets)``: every frame's deflate body packed back
    to back in the uint8 buffer ``out`` (frame f at ``offsets[f]``, int64 [F]) and int32 ``meta``: ``meta[:F]`` the bodies' byte
    counts, ``meta[F:]`` viewed as [F, stripes, 2] the Adler-32 halves (s1, s2) of every stripe's bytes -- one small copy gives the host
    all it needs besides ``out[:lengths.sum()]``.  Stripes of ``stripe_rows`` rows are coded independently: one dynamic-Huffman
    block of literals and distance-1 matches closed by an empty stored block, or stored blocks where that is not smaller; ``03 00``
    ends a body (csrc/png.hip; ``tests/png_model.deflate_rows`` byte for byte).  ``out``: a contiguous uint8 buffer, by default
    F x ``png_deflate_bound``.  Bytes that a smaller ``out`` cannot hold are dropped, and the caller sees it from the lengths."""
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.uint8 or rows.dim() != 3 or not rows.is_contiguous():
        raise VFaceHipError("png_deflate: rows must be a contiguous uint8 [F, H, row_bytes] tensor on the GPU")
    F_, H, rb = rows.shape
    stripe_rows = int(stripe_rows)
    if min(F_, H, rb) <= 0 or stripe_rows <= 0:
        raise VFaceHipError(f"png_deflate: F, H, row_bytes and stripe_rows must be positive; got {F_}, {H}, {rb}, {stripe_rows}")
    if rb * H >= 1 << 31 or png_deflate_bound(rb, H, stripe_rows) >= 1 << 31:
        raise VFaceHipError(f"png_deflate: a frame's rows and its bound stay below 2^31 bytes; got {rb} x {H}")
    if out is None:
        out = torch.empty(F_ * png_deflate_bound(rb, H, stripe_rows), dtype=torch.uint8, device=rows.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != rows.device or out.numel() == 0:
        raise VFaceHipError("png_deflate: out must be a contiguous uint8 buffer on the rows' device")
    lib = load()
    need = int(lib.vface_png_deflate_workspace_bytes(rb, H, F_, stripe_rows))
    ws = _png_ws.get(str(rows.device))
    if ws is None or ws.numel() < need:
        ws = _png_ws[str(rows.device)] = torch.empty(need, dtype=torch.uint8, device=rows.device)
    stripes = (H + stripe_rows - 1) // stripe_rows
    meta = torch.empty(F_ + 2 * F_ * stripes, dtype=torch.int32, device=rows.device)
    offsets = torch.empty(F_, dtype=torch.int64, device=rows.device)
    _check(lib.vface_png_deflate(_p(rows), rb, H, F_, stripe_rows, _p(out), out.numel(), _p(offsets), _p(meta), _p(meta[F_:]), _p(ws),
                                 ws.numel(), _stream()), "vface_png_deflate")
    return out, meta, offsets


# ---- GIF out (:658; csrc/gif.hip)
GIF_SEG_PIXELS = 16384             # indices of a frame that one wave codes from an empty table: tools/bench_gif.py's sweep over 1024 .. 16384
                                   # (profiles/r14_a_*): the LZW pass for 32 frames of 1920 x 1080 takes the same time at every length (22.2 ..
                                   # 23.0 ms), and the image data shrinks from 680 kB (1024) over 534 kB (4096) to 350 kB per smooth frame, 906 /
                                   # 777 / 586 kB per noisy one, where Pillow's one stream takes 298 / 587 kB; one frame alone pays 4.5 ms
                                   # instead of 1.3
GIF_CELLS, GIF_COLORS = 32768, 256
GIF_MAX_SIDE, GIF_MAX_PIXELS = 65535, 1 << 24      # kGifMaxSide, kGifMaxPixels: a box's channel sum, at most 255 * 2^24, fits 32 bits
GIF_MAX_SEG_PIXELS = 65535
GIF_HIST_SHARE, GIF_HIST_GRID_CAP = 65536, 1024    # kGifHistShare pixels per workgroup; workgroups before the grid loops
GIF_BOXES_GRID_CAP = 64                            # kGifBoxesGridCap: workgroups, one frame each
GIF_PALETTE_SHARE, GIF_PALETTE_GRID_CAP = 16384, 2048
GIF_MAP_SHARE, GIF_MAP_GRID_CAP = 8192, 4096
GIF_LZW_GRID_CAP = 4096                            # kGifLzwGridCap: workgroups of one wave, one (frame, segment) each
GIF_LZW_FLAT_GRID_CAP = 2048                       # kGifFlatGridCap: workgroups of 256 codes (the pack) or bytes (the framing)
_gif_ws = {}


def _gif_frames(frames_u8, what):
    if (not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4
            or frames_u8.shape[-1] != 3 or not frames_u8.is_contiguous()):
        raise VFaceHipError(f"{what}: frames must be contiguous uint8 [F, H, W, 3] on the GPU")
    F_, H, W, _ = frames_u8.shape
    if F_ <= 0 or not (1 <= W <= GIF_MAX_SIDE and 1 <= H <= GIF_MAX_SIDE) or W * H > GIF_MAX_PIXELS:
        raise VFaceHipError(f"{what}: F >= 1, W and H in 1..{GIF_MAX_SIDE} and W * H <= 2^24 (the histogram's 32-bit bound); got {F_}, {W} x {H}")
    return F_, H, W


def _gif_buffer(t, dtype, shape, device, what):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        raise VFaceHipError(f"{what} must be a contiguous {dtype} {list(shape)} tensor on the frames' device")
    return t


def gif_histogram(frames_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 device frames [F, H, W, 3] -> int32 [F, 32768] (read as unsigned): the pixels in every cell of 8 x 8 x 8,
    cell = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) (:658; csrc/gif.hip; ``tests/gif_model.histogram``)."""
    F_, H, W = _gif_frames(frames_u8, "gif_histogram")
    out = _gif_buffer(out, torch.int32, (F_, GIF_CELLS), frames_u8.device, "gif_histogram: out")
    _check(load().vface_gif_histogram(_p(frames_u8), W, H, F_, _p(out), _stream()), "vface_gif_histogram")
    return out


def gif_boxes(counts: torch.Tensor, labels: Optional[torch.Tensor] = None, ncolors: Optional[torch.Tensor] = None):
    """``gif_histogram``'s counts [F, 32768] -> ``(labels, ncolors)``: uint8 [F, 32768], the median-cut box of every cell (0 for an empty
    cell), and int32 [F], the number of boxes.  The rule is csrc/gif_palette.hpp's (``tests/gif_model.boxes`` bit for bit)."""
    if (not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype != torch.int32 or counts.dim() != 2
            or counts.shape[1] != GIF_CELLS or counts.shape[0] <= 0 or not counts.is_contiguous()):
        raise VFaceHipError(f"gif_boxes: counts must be a contiguous int32 [F, {GIF_CELLS}] tensor on the GPU")
    F_ = counts.shape[0]
    labels = _gif_buffer(labels, torch.uint8, (F_, GIF_CELLS), counts.device, "gif_boxes: labels")
    ncolors = _gif_buffer(ncolors, torch.int32, (F_,), counts.device, "gif_boxes: ncolors")
    _check(load().vface_gif_boxes(_p(counts), F_, _p(labels), _p(ncolors), _stream()), "vface_gif_boxes")
    return labels, ncolors


def gif_palette(frames_u8: torch.Tensor, labels: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Frames and ``gif_boxes``' labels -> uint8 [F, 256, 3]: entry i is the mean, halves up, of the pixels whose cell lies in box i;
    entries without pixels are zeros (``tests/gif_model.palette``)."""
    F_, H, W = _gif_frames(frames_u8, "gif_palette")
    labels = _gif_buffer(labels, torch.uint8, (F_, GIF_CELLS), frames_u8.device, "gif_palette: labels")
    out = _gif_buffer(out, torch.uint8, (F_, GIF_COLORS, 3), frames_u8.device, "gif_palette: out")
    sums = torch.empty((F_, GIF_COLORS, 4), dtype=torch.int32, device=frames_u8.device)
    _check(load().vface_gif_palette(_p(frames_u8), W, H, F_, _p(labels), _p(out), _p(sums), _stream()), "vface_gif_palette")
    return out


def gif_map(frames_u8: torch.Tensor, palette: torch.Tensor, ncolors: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Frames, palettes [F, 256, 3] and ncolors [F] -> uint8 [F, H * W]: every pixel's palette entry of smallest squared RGB distance
    among the first ncolors, the lowest index on a tie; exact search (``tests/gif_model.index_map``)."""
    F_, H, W = _gif_frames(frames_u8, "gif_map")
    palette = _gif_buffer(palette, torch.uint8, (F_, GIF_COLORS, 3), frames_u8.device, "gif_map: palette")
    ncolors = _gif_buffer(ncolors, torch.int32, (F_,), frames_u8.device, "gif_map: ncolors")
    out = _gif_buffer(out, torch.uint8, (F_, H * W), frames_u8.device, "gif_map: out")
    _check(load().vface_gif_map(_p(frames_u8), W, H, F_, _p(palette), _p(ncolors), _p(out), _stream()), "vface_gif_map")
    return out


def gif_lzw_bound(npix: int, seg_pixels: int = GIF_SEG_PIXELS) -> int:
    """Bytes that always hold one frame's image data: every segment at the most codes it can make, the sub-block framing."""
    n = int(load().vface_gif_lzw_bound(int(npix), int(seg_pixels)))
    if n == 0:
        raise VFaceHipError(f"gif_lzw: npix is 1..2^24 and seg_pixels 1..{GIF_MAX_SEG_PIXELS}; got {npix}, {seg_pixels}")
    return n


def gif_lzw(indices: torch.Tensor, seg_pixels: int = GIF_SEG_PIXELS, out: Optional[torch.Tensor] = None):
    """Index maps, device uint8 [F, npix] -> ``(out, offsets)``: every frame's GIF image data (08, the LZW stream in sub-blocks, 00)
    packed back to back in the uint8 buffer ``out``, frame f at ``out[offsets[f]:offsets[f + 1]]`` (int64 [F + 1]).  Segments of
    ``seg_pixels`` indices are coded from an empty table by one wave each and end in a Clear (csrc/gif.hip;
    ``tests/gif_model.image_data`` byte for byte).  ``out``: a contiguous uint8 buffer, by default F x ``gif_lzw_bound``.  Bytes that
    a smaller ``out`` cannot hold are dropped; the caller sees it from ``offsets[F] > out.numel()``."""
    if not isinstance(indices, torch.Tensor) or not indices.is_cuda or indices.dtype != torch.uint8 or indices.dim() != 2 or not indices.is_contiguous():
        raise VFaceHipError("gif_lzw: indices must be a contiguous uint8 [F, npix] tensor on the GPU")
    F_, npix = indices.shape
    seg_pixels = int(seg_pixels)
    if F_ <= 0 or not 1 <= npix <= GIF_MAX_PIXELS or not 1 <= seg_pixels <= GIF_MAX_SEG_PIXELS:
        raise VFaceHipError(f"gif_lzw: F >= 1, npix in 1..2^24 and seg_pixels in 1..{GIF_MAX_SEG_PIXELS}; got {F_}, {npix}, {seg_pixels}")
    if out is None:
        out = torch.empty(F_ * gif_lzw_bound(npix, seg_pixels), dtype=torch.uint8, device=indices.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != indices.device or out.numel() == 0:
        raise VFaceHipError("gif_lzw: out must be a contiguous uint8 buffer on the indices' device")
    lib = load()
    need = int(lib.vface_gif_lzw_workspace_bytes(npix, F_, seg_pixels))
    ws = _gif_ws.get(str(indices.device))
    if ws is None or ws.numel() < need:
        ws = _gif_ws[str(indices.device)] = torch.empty(need, dtype=torch.uint8, device=indices.device)
    offsets = torch.empty(F_ + 1, dtype=torch.int64, device=indices.device)
    _check(lib.vface_gif_lzw(_p(indices), npix, F_, seg_pixels, _p(out), out.numel(), _p(offsets), _p(ws), ws.numel(), _stream()),
           "vface_gif_lzw")
    return out, offsets


# ---- PNG frames in (:285; csrc/png_in.hip)
PNG_UNFILTER_MAX_W = 8192          # kUnfilterMaxW: the row carried from one band of 64 rows to the next lives in LDS
PNG_INFLATE_GRID_CAP = 1024        # kInflateGridCap: workgroups, one file each, before the grid loops


def _is_dev(t, dtype, dim=None):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and (dim is None or t.dim() == dim)


def png_inflate(streams: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, expect: int, out: Optional[torch.Tensor] = None,
                meta: Optional[torch.Tensor] = None):
    """Raw deflate bodies (RFC 1951), file f the ``lengths[f]`` (int32 [F]) bytes at ``offsets[f]`` (int64 [F]) of the uint8 device
    buffer ``streams`` -> ``(rows, meta)``: uint8 [F, expect], each file's bytes, and int32 ``meta`` [5, F]: status, produced,
    consumed, and in ``meta[3:]`` viewed as [F, 2] the Adler-32 halves (s1, s2) of the produced bytes.  Status 0: the final block
    ended with exactly ``expect`` bytes; 1..14 name what stopped the stream first (``scripts/png_in.INFLATE_STATUS``); such a file's
    row holds the ``produced`` bytes made before, and nothing is written behind them.  One wave per file (csrc/png_in.hip;
    ``tests/png_inflate_model.inflate`` bit for bit).  ``out``: a uint8 [F, >= expect] buffer; ``meta``: an int32 [5, F] one."""
    if not _is_dev(streams, torch.uint8, 1) or streams.numel() == 0:
        raise VFaceHipError("png_inflate: streams must be a contiguous uint8 buffer on the GPU, at least one byte")
    if not _is_dev(offsets, torch.int64, 1) or not _is_dev(lengths, torch.int32, 1) or offsets.numel() != lengths.numel() or offsets.numel() == 0:
        raise VFaceHipError("png_inflate: offsets (int64) and lengths (int32) must be contiguous [F] tensors on the GPU, F >= 1")
    if offsets.device != streams.device or lengths.device != streams.device:
        raise VFaceHipError("png_inflate: streams, offsets and lengths must be on one device")
    F_, expect = offsets.numel(), int(expect)
    if not 0 < expect < 1 << 31 or streams.numel() >= 1 << 31:
        raise VFaceHipError(f"png_inflate: expect and the stream buffer are 1 .. 2^31 - 1 bytes; got {expect}, {streams.numel()}")
    if out is None:
        out = torch.empty((F_, expect), dtype=torch.uint8, device=streams.device)
    elif not _is_dev(out, torch.uint8, 2) or out.shape[0] != F_ or out.shape[1] < expect or out.device != streams.device:
        raise VFaceHipError(f"png_inflate: out must be a contiguous uint8 [{F_}, >= {expect}] tensor on the streams' device")
    if meta is None:
        meta = torch.empty((5, F_), dtype=torch.int32, device=streams.device)
    elif not _is_dev(meta, torch.int32, 2) or tuple(meta.shape) != (5, F_) or meta.device != streams.device:
        raise VFaceHipError(f"png_inflate: meta must be a contiguous int32 [5, {F_}] tensor on the streams' device")
    _check(load().vface_png_inflate(_p(streams), streams.numel(), _p(offsets), _p(lengths), F_, _p(out), out.shape[1], expect, _p(meta[0]),
                                    _p(meta[1]), _p(meta[2]), _p(meta[3]), _stream()), "vface_png_inflate")
    return out, meta


def png_unfilter(rows: torch.Tensor, W: int, H: int, bpp: int, inflate_status: torch.Tensor, out: Optional[torch.Tensor] = None,
                 status: Optional[torch.Tensor] = None):
    """Filtered rows, device uint8 [F, >= H (1 + bpp W)] (``png_inflate``'s rows) -> ``(rgb, status)``: uint8 [F, H, W, 3] and int32
    [F]: 0, or 1 + the first row whose filter byte is above 4.  bpp 3 = RGB, 4 = RGBA (alpha dropped), 1 = grey (replicated).  A
    file whose ``inflate_status`` (int32 [F]) is not 0 is not read; its frame, like that of a file with a bad filter byte, is
    zeros (csrc/png_in.hip; ``tests/png_inflate_model.unfilter`` bit for bit)."""
    W, H, bpp = int(W), int(H), int(bpp)
    if bpp not in (1, 3, 4) or min(W, H) <= 0:
        raise VFaceHipError(f"png_unfilter: W and H must be positive and bpp 1, 3 or 4; got {W}, {H}, {bpp}")
    need = (1 + bpp * W) * H
    if need >= 1 << 31 or W > PNG_UNFILTER_MAX_W:
        raise VFaceHipError(f"png_unfilter: a frame's rows stay below 2^31 bytes and W at or below {PNG_UNFILTER_MAX_W}; got {W} x {H}")
    if not _is_dev(rows, torch.uint8, 2) or rows.shape[0] == 0 or rows.shape[1] < need:
        raise VFaceHipError(f"png_unfilter: rows must be a contiguous uint8 [F, >= {need}] tensor on the GPU")
    F_ = rows.shape[0]
    if not _is_dev(inflate_status, torch.int32, 1) or inflate_status.numel() != F_ or inflate_status.device != rows.device:
        raise VFaceHipError(f"png_unfilter: inflate_status must be a contiguous int32 [{F_}] tensor on the rows' device")
    if out is None:
        out = torch.empty((F_, H, W, 3), dtype=torch.uint8, device=rows.device)
    elif not _is_dev(out, torch.uint8, 4) or tuple(out.shape) != (F_, H, W, 3) or out.device != rows.device:
        raise VFaceHipError(f"png_unfilter: out must be a contiguous uint8 [{F_}, {H}, {W}, 3] tensor on the rows' device")
    if status is None:
        status = torch.empty(F_, dtype=torch.int32, device=rows.device)
    elif not _is_dev(status, torch.int32, 1) or status.numel() != F_ or status.device != rows.device:
        raise VFaceHipError(f"png_unfilter: status must be a contiguous int32 [{F_}] tensor on the rows' device")
    _check(load().vface_png_unfilter(_p(rows), rows.shape[1], W, H, bpp, F_, _p(inflate_status), _p(out), _p(status), _stream()),
           "vface_png_unfilter")
    return out, status


PNG_INFLATE_CHUNK_BYTES = 16384    # compressed bytes per chunk of png_inflate_parallel: zlib's level-6 streams of noisy frames start a block about
                                   # every 16 KiB, so a chunk holds about one block start (tools/bench_png_in.py sweeps 4 .. 64 KiB)
PNG_INFLATE_PAR_DECODE_GRID_CAP = 2048     # kFindGridCap, kCountGridCap (kWriteGridCap is 1024): workgroups of one wave before the grid loops
PNG_INFLATE_PAR_RESOLVE_GRID_CAP = 256     # kResolveGridCap: workgroups, one file each
PNG_INFLATE_FALLBACK_REASONS = {0: "none", 1: "the chain of segments did not close", 2: "a segment reported a status",
                                3: "the byte count is not the image's", 4: "a distance reaches in front of the file",
                                5: "the file's range lies outside the buffer"}
_png_par_ws = {}


def png_inflate_parallel_workspace_bytes(files: int, stream_bytes: int, expect: int, chunk_bytes: int = PNG_INFLATE_CHUNK_BYTES) -> int:
    """Bytes of workspace ``vface_png_inflate_parallel`` asks for: the segment tables of ``files * ceil(stream_bytes / chunk_bytes)``
    entries and two bytes per output byte."""
    need = int(load().vface_png_inflate_parallel_workspace_bytes(int(files), int(stream_bytes), int(expect), int(chunk_bytes)))
    if need == 0:
        raise VFaceHipError(f"png_inflate_parallel: files, stream_bytes and expect are 1 .. 2^31 - 1 and chunk_bytes a multiple of 4 in "
                            f"64 .. 2^20; got {files}, {stream_bytes}, {expect}, {chunk_bytes}")
    return need


def png_inflate_parallel(streams: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, expect: int,
                         chunk_bytes: int = PNG_INFLATE_CHUNK_BYTES, out: Optional[torch.Tensor] = None, meta: Optional[torch.Tensor] = None,
                         info: Optional[torch.Tensor] = None):
    """``png_inflate`` with many waves per file -> ``(rows, meta, info)``: rows and meta are ``png_inflate``'s bit for bit, for every
    input.  A file's body is cut into chunks of ``chunk_bytes``; a chunk in which a dynamic block starts begins a segment there, one
    wave per segment counts and then decodes it into 16-bit elements, and the segments are resolved in order
    (csrc/png_in_par.hip; ``tests/png_inflate_par_model.inflate_parallel``).  A file whose segments do not chain up exactly is
    decoded by ``png_inflate``'s kernel in the same call.  ``info``: int32 [F, 4]: segments decoded in parallel (0: the serial
    kernel decoded the file), why it did (``PNG_INFLATE_FALLBACK_REASONS``), candidates found, 0.  The workspace is kept here, per
    device, and grown when needed."""
    chunk_bytes = int(chunk_bytes)
    if not 64 <= chunk_bytes <= 1 << 20 or chunk_bytes % 4:
        raise VFaceHipError(f"png_inflate_parallel: chunk_bytes must be a multiple of 4 in 64 .. 2^20; got {chunk_bytes}")
    if not _is_dev(streams, torch.uint8, 1) or streams.numel() == 0:
        raise VFaceHipError("png_inflate_parallel: streams must be a contiguous uint8 buffer on the GPU, at least one byte")
    if not _is_dev(offsets, torch.int64, 1) or not _is_dev(lengths, torch.int32, 1) or offsets.numel() != lengths.numel() or offsets.numel() == 0:
        raise VFaceHipError("png_inflate_parallel: offsets (int64) and lengths (int32) must be contiguous [F] tensors on the GPU, F >= 1")
    if offsets.device != streams.device or lengths.device != streams.device:
        raise VFaceHipError("png_inflate_parallel: streams, offsets and lengths must be on one device")
    F_, expect = offsets.numel(), int(expect)
    if not 0 < expect < 1 << 31 or streams.numel() >= 1 << 31:
        raise VFaceHipError(f"png_inflate_parallel: expect and the stream buffer are 1 .. 2^31 - 1 bytes; got {expect}, {streams.numel()}")
    if out is None:
        out = torch.empty((F_, expect), dtype=torch.uint8, device=streams.device)
    elif not _is_dev(out, torch.uint8, 2) or out.shape[0] != F_ or out.shape[1] < expect or out.device != streams.device:
        raise VFaceHipError(f"png_inflate_parallel: out must be a contiguous uint8 [{F_}, >= {expect}] tensor on the streams' device")
    if meta is None:
        meta = torch.empty((5, F_), dtype=torch.int32, device=streams.device)
    elif not _is_dev(meta, torch.int32, 2) or tuple(meta.shape) != (5, F_) or meta.device != streams.device:
        raise VFaceHipError(f"png_inflate_parallel: meta must be a contiguous int32 [5, {F_}] tensor on the streams' device")
    if info is None:
        info = torch.empty((F_, 4), dtype=torch.int32, device=streams.device)
    elif not _is_dev(info, torch.int32, 2) or tuple(info.shape) != (F_, 4) or info.device != streams.device:
        raise VFaceHipError(f"png_inflate_parallel: info must be a contiguous int32 [{F_}, 4] tensor on the streams' device")
    need = png_inflate_parallel_workspace_bytes(F_, streams.numel(), expect, chunk_bytes)
    ws = _png_par_ws.get(str(streams.device))
    if ws is None or ws.numel() < need:
        ws = _png_par_ws[str(streams.device)] = torch.empty(need, dtype=torch.uint8, device=streams.device)
    _check(load().vface_png_inflate_parallel(_p(streams), streams.numel(), _p(offsets), _p(lengths), F_, _p(out), out.shape[1], expect,
                                             _p(meta[0]), _p(meta[1]), _p(meta[2]), _p(meta[3]), chunk_bytes, _p(ws), ws.numel(), _p(info),
                                             _stream()), "vface_png_inflate_parallel")
    return out, meta, info


YUV_MATRICES = {"bt709": 0, "bt601": 1}
YUV_CHROMA = {"nearest": 0, "centre": 1, "left": 2}


def yuv420_to_rgb(i420: torch.Tensor, W: int, H: int, matrix: str = "bt709", full_range: bool = False, chroma: str = "centre",
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """I420 frames, device uint8 [F, n >= frame_bytes] rows (Y [H][W], Cb [ch][cw], Cr [ch][cw]; a view with a row stride is fine,
    the bytes past frame_bytes are not read) -> uint8 [F, H, W, 3] RGB: the inverse direction of ``rgb_to_yuv420``, the integer
    arithmetic of ``tests/demux_model.py`` bit for bit (csrc/demux.hip).  ``matrix``: bt709 | bt601; ``full_range``: limited (tv)
    or full; ``chroma``: nearest | centre (C420jpeg, what ``rgb_to_yuv420`` writes) | left (C420mpeg2).  ``out``: a contiguous
    uint8 [F, H, W, 3] tensor on the frames' device."""
    if matrix not in YUV_MATRICES:
        raise VFaceHipError(f"yuv420_to_rgb: matrix is one of {sorted(YUV_MATRICES)}; got {matrix!r}")
    if chroma not in YUV_CHROMA:
        raise VFaceHipError(f"yuv420_to_rgb: chroma is one of {sorted(YUV_CHROMA)}; got {chroma!r}")
    W, H = int(W), int(H)
    if not isinstance(i420, torch.Tensor) or i420.dtype != torch.uint8 or i420.dim() != 2:
        raise VFaceHipError("yuv420_to_rgb: frames must be uint8 [F, >= frame_bytes] rows")
    F_ = i420.shape[0]
    if min(F_, H, W) <= 0:
        raise VFaceHipError("yuv420_to_rgb: F, H and W must be positive")
    n = i420_frame_bytes(W, H)
    if i420.shape[1] < n or i420.stride(1) != 1 or (F_ > 1 and i420.stride(0) < n):
        raise VFaceHipError(f"yuv420_to_rgb: a {W} x {H} I420 frame is {n} bytes; frames must be rows of at least that many bytes with "
                            f"unit column stride, row stride >= {n}; got {tuple(i420.shape)}, strides {tuple(i420.stride())}")
    if out is None:
        out = torch.empty(F_, H, W, 3, dtype=torch.uint8, device=i420.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F_, H, W, 3) or not out.is_contiguous() or out.device != i420.device:
        raise VFaceHipError(f"yuv420_to_rgb: out must be a contiguous uint8 {[F_, H, W, 3]} tensor on the frames' device")
    stride = i420.stride(0) if F_ > 1 else max(i420.stride(0), n)
    _check(load().vface_yuv420_to_rgb(_p(i420), stride, W, H, F_, _p(out), YUV_MATRICES[matrix], int(bool(full_range)),
                                      YUV_CHROMA[chroma], _stream()), "vface_yuv420_to_rgb")
    return out


JPEG_TABLE_BYTES = 6 * (16 * 4 + 16 * 4 + 256)      # a frame's Huffman tables as the decoder reads them (csrc/jpeg_interval.hpp)
JPEG_STATUS = {0: "decoded", 1: "the scan does not hold the RST markers its DRI promises", 2: "the RST markers are out of order",
               3: "the bytes of a restart interval ran out before its blocks", 4: "bits that are no code of the frame's Huffman table",
               5: "a DC difference category above 11", 6: "an AC coefficient size above 10", 7: "a zero run past coefficient 63",
               8: "a DC value outside 16 bits"}


def jpeg_interval_count(mcus: int, restart: int) -> int:
    """Restart intervals of a frame of ``mcus`` MCUs whose DRI says ``restart`` (0 = none)."""
    mcus, restart = int(mcus), int(restart)
    return 1 if restart <= 0 or restart >= mcus else -(-mcus // restart)


def _jpeg_in_frames(what, scans, restart, mcus, max_intervals):
    if not isinstance(scans, torch.Tensor) or scans.dtype != torch.uint8 or scans.dim() != 1 or not scans.is_contiguous() or scans.numel() == 0:
        raise VFaceHipError(f"{what}: scans must be a contiguous, non-empty uint8 buffer")
    if (not isinstance(restart, torch.Tensor) or restart.dtype != torch.int32 or restart.dim() != 1 or not restart.is_contiguous()
            or restart.device != scans.device or restart.numel() == 0):
        raise VFaceHipError(f"{what}: restart must be a contiguous int32 [F] tensor on the scans' device, F > 0")
    mcus, max_intervals = int(mcus), int(max_intervals)
    if mcus <= 0 or not 1 <= max_intervals <= mcus:
        raise VFaceHipError(f"{what}: mcus must be positive and max_intervals in 1..mcus; got {mcus}, {max_intervals}")
    if scans.numel() >= 2 ** 31:
        raise VFaceHipError(f"{what}: the scans of one call must stay under 2 GiB; got {scans.numel()} bytes")
    return restart.numel(), mcus, max_intervals


def jpeg_scan_index(scans: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, restart: torch.Tensor, mcus: int,
                    max_intervals: int, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The restart intervals of every frame's scan.  ``scans``: device uint8, the entropy-coded segments of F frames in one
    buffer; ``offsets`` int64 [F], ``lengths`` int32 [F]: where each lies; ``restart`` int32 [F]: each frame's DRI value, 0 = none;
    ``mcus``: MCUs per frame; ``max_intervals`` >= every frame's ``jpeg_interval_count``.  -> ``(ranges, status)``: int32
    [F, max_intervals, 2] (begin, end) in bytes of ``scans``, the RST markers in neither, zeros past a frame's count; int32 [F],
    0 or 1 = wrong marker count, 2 = wrong marker order (``JPEG_STATUS``), and such a frame's ranges are zeros.  csrc/mjpeg_in.hip."""
    F_, mcus, max_intervals = _jpeg_in_frames("jpeg_scan_index", scans, restart, mcus, max_intervals)
    for name, t, dt in (("offsets", offsets, torch.int64), ("lengths", lengths, torch.int32)):
        if (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (F_,) or not t.is_contiguous()
                or t.device != scans.device):
            raise VFaceHipError(f"jpeg_scan_index: {name} must be a contiguous {dt} [{F_}] tensor on the scans' device")
    if out is None:
        out = torch.empty(F_, max_intervals, 2, dtype=torch.int32, device=scans.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (F_, max_intervals, 2) or not out.is_contiguous() or out.device != scans.device:
        raise VFaceHipError(f"jpeg_scan_index: out must be a contiguous int32 {[F_, max_intervals, 2]} tensor on the scans' device")
    status = torch.empty(F_, dtype=torch.int32, device=scans.device)
    _check(load().vface_jpeg_scan_index(_p(scans), scans.numel(), _p(offsets), _p(lengths), _p(restart), mcus, F_, max_intervals,
                                        _p(out), _p(status), _stream()), "vface_jpeg_scan_index")
    return out, status


def _jpeg_decode_args(what, scans, ranges, status, restart, tables, mcus, out):
    """The checks ``jpeg_decode_entropy`` and ``jpeg_decode_entropy_parallel`` share -> (F, mcus, max_intervals, out, frame stride)."""
    if not isinstance(ranges, torch.Tensor) or ranges.dim() != 3:
        raise VFaceHipError(f"{what}: ranges must be int32 [F, max_intervals, 2]")
    F_, mcus, max_intervals = _jpeg_in_frames(what, scans, restart, mcus, ranges.shape[1])
    if ranges.dtype != torch.int32 or tuple(ranges.shape) != (F_, max_intervals, 2) or not ranges.is_contiguous() or ranges.device != scans.device:
        raise VFaceHipError(f"{what}: ranges must be a contiguous int32 {[F_, max_intervals, 2]} tensor on the scans' device")
    if (not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or tuple(status.shape) != (F_,) or not status.is_contiguous()
            or status.device != scans.device):
        raise VFaceHipError(f"{what}: status must be a contiguous int32 [{F_}] tensor on the scans' device")
    if (not isinstance(tables, torch.Tensor) or tables.dtype != torch.uint8 or tuple(tables.shape) != (F_, JPEG_TABLE_BYTES)
            or not tables.is_contiguous() or tables.device != scans.device):
        raise VFaceHipError(f"{what}: tables must be a contiguous uint8 {[F_, JPEG_TABLE_BYTES]} tensor on the scans' device")
    shape, n = (F_, mcus, 6, 64), mcus * JPEG_MCU_COEFS
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=scans.device)
    elif (out.dtype != torch.int16 or tuple(out.shape) != shape or not out[0].is_contiguous() or (F_ > 1 and out.stride(0) < n)
          or out.device != scans.device):
        raise VFaceHipError(f"{what}: out must be an int16 {list(shape)} view on the scans' device, frames contiguous, "
                            f"frame stride >= {n}")
    return F_, mcus, max_intervals, out, out.stride(0) if F_ > 1 else max(out.stride(0), n)


def jpeg_decode_entropy(scans: torch.Tensor, ranges: torch.Tensor, status: torch.Tensor, restart: torch.Tensor,
                        tables: torch.Tensor, mcus: int, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ranges`` and ``status`` of ``jpeg_scan_index`` -> ``(coefficients, status)``: int16 [F, mcus, 6, 64], the layout
    ``jpeg_coefficients`` writes (blocks Y00 Y01 Y10 Y11 Cb Cr, zigzag order), so ``jpeg_entropy`` followed by this is the identity;
    ``status`` is updated in place: the largest code of a frame's intervals (``JPEG_STATUS``).  ``tables``: device uint8
    [F, JPEG_TABLE_BYTES], every frame's Huffman tables by component (``scripts/mjpeg_in.huffman_block``).  One lane decodes one
    interval with the routine of csrc/jpeg_interval.hpp: no byte outside an interval is read and no element outside its MCUs is
    written, whatever the bytes are.  Every frame is cleared first; a refused frame stays zero.  ``out``: an int16 view
    [F, mcus, 6, 64] with contiguous frames, frame stride at least one frame; elements between frames are not written."""
    F_, mcus, max_intervals, out, stride = _jpeg_decode_args("jpeg_decode_entropy", scans, ranges, status, restart, tables, mcus, out)
    _check(load().vface_jpeg_decode_entropy(_p(scans), scans.numel(), _p(ranges), _p(restart), _p(tables), mcus, F_, max_intervals,
                                            _p(out), stride, _p(status), _stream()), "vface_jpeg_decode_entropy")
    return out, status


JPEG_PARALLEL_LANES = (64, 256)     # lanes (subsequences) per chunk of the two instantiations (csrc/jpeg_subseq.hpp)
_jpeg_parallel_ws = {}


def jpeg_parallel_lanes(scan_bytes: int, frames: int, max_intervals: int, subseq_bytes: int) -> int:
    """Lanes per chunk ``vface_jpeg_decode_entropy_parallel`` picks for a call (``vf_jpeg_subseq_lanes`` of csrc/jpeg_subseq.hpp, the
    same integer arithmetic): the long form once the average interval holds at least as many subsequences as the short form has
    lanes.  ``rounds`` depends on it, the coefficients do not."""
    intervals = max(int(frames) * int(max_intervals), 1)
    return JPEG_PARALLEL_LANES[1] if int(scan_bytes) // intervals // int(subseq_bytes) >= JPEG_PARALLEL_LANES[0] else JPEG_PARALLEL_LANES[0]


def jpeg_decode_entropy_parallel(scans: torch.Tensor, ranges: torch.Tensor, status: torch.Tensor, restart: torch.Tensor,
                                 tables: torch.Tensor, mcus: int, subseq_bytes: int = 256, out: Optional[torch.Tensor] = None,
                                 return_rounds: bool = False):
    """``jpeg_decode_entropy``'s arguments and result -- the same coefficients and statuses for every input, valid or corrupt --
    from many lanes per restart interval: the interval is cut into subsequences of ``subseq_bytes`` raw scan bytes (a multiple of
    4 in 4..1024; 256 is what tools/bench_mjpeg_in.py's sweep chose), one workgroup decodes them from guessed states, chunk by chunk, and stitches them by self-synchronisation; DC
    values come from a prefix sum of the differences; a frame the serial routine would refuse is decoded again by the serial
    routine itself (csrc/jpeg_subseq.hpp, csrc/mjpeg_in.hip).  For scans without restart markers, where ``jpeg_decode_entropy``
    has one lane per frame.  ``return_rounds``: also int32 [F, max_intervals], the synchronisation rounds that changed a state,
    summed over an interval's chunks (at most its subsequences minus its chunks: a stream that never synchronises)."""
    F_, mcus, max_intervals, out, stride = _jpeg_decode_args("jpeg_decode_entropy_parallel", scans, ranges, status, restart, tables,
                                                             mcus, out)
    subseq_bytes = int(subseq_bytes)
    if not 4 <= subseq_bytes <= 1024 or subseq_bytes % 4:
        raise VFaceHipError(f"jpeg_decode_entropy_parallel: subseq_bytes must be a multiple of 4 in 4..1024; got {subseq_bytes}")
    lib = load()
    need = int(lib.vface_jpeg_decode_entropy_parallel_workspace_bytes(F_))
    ws = _jpeg_parallel_ws.get(str(scans.device))
    if ws is None or ws.numel() < need:
        ws = _jpeg_parallel_ws[str(scans.device)] = torch.empty(need, dtype=torch.uint8, device=scans.device)
    rounds = torch.empty(F_, max_intervals, dtype=torch.int32, device=scans.device) if return_rounds else None
    _check(lib.vface_jpeg_decode_entropy_parallel(_p(scans), scans.numel(), _p(ranges), _p(restart), _p(tables), mcus, F_, max_intervals,
                                                  _p(out), stride, _p(status), subseq_bytes, _p(ws), ws.numel(), _p(rounds), _stream()),
           "vface_jpeg_decode_entropy_parallel")
    return (out, status, rounds) if return_rounds else (out, status)


def jpeg_planes(coef: torch.Tensor, quant: torch.Tensor, W: int, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Coefficient frames, device int16 [F, mcus, 6, 64] (or [F, mcu_rows, mcu_cols, 6, 64]; a frame stride is fine) and ``quant``,
    device uint8 [F, 3, 64]: every frame's quantisation tables of Y, Cb, Cr, row-major -> uint8 [F, frame_bytes] I420 rows of
    the W x H frames (Y [H][W], Cb [ch][cw], Cr [ch][cw]), what ``yuv420_to_rgb`` reads.  Dequantisation, integer inverse DCT,
    + 128, clamp, crop: the arithmetic of ``tests/jpeg_decode_model.py``, bit for bit (csrc/mjpeg_in.hip).  ``out``: a uint8 view
    [F, n >= frame_bytes] with unit column stride; bytes past frame_bytes of a row are not written."""
    if (not isinstance(coef, torch.Tensor) or coef.dtype != torch.int16 or coef.dim() not in (4, 5) or tuple(coef.shape[-2:]) != (6, 64)
            or coef.shape[0] == 0 or not coef[0].is_contiguous()):
        raise VFaceHipError("jpeg_planes: coefficients must be int16 [F, mcus, 6, 64] with contiguous frames, F > 0")
    W, H = int(W), int(H)
    F_, mcus = coef.shape[0], coef[0].numel() // JPEG_MCU_COEFS
    mr, mc = jpeg_mcu_grid(W, H)
    if min(W, H) <= 0 or mcus != mr * mc:
        raise VFaceHipError(f"jpeg_planes: a {W} x {H} frame is {mr} x {mc} MCUs; the coefficients hold {mcus} per frame")
    n = mcus * JPEG_MCU_COEFS
    if F_ > 1 and coef.stride(0) < n:
        raise VFaceHipError(f"jpeg_planes: frame stride >= {n}")
    if (not isinstance(quant, torch.Tensor) or quant.dtype != torch.uint8 or tuple(quant.shape) != (F_, 3, 64) or not quant.is_contiguous()
            or quant.device != coef.device):
        raise VFaceHipError(f"jpeg_planes: quant must be a contiguous uint8 {[F_, 3, 64]} tensor on the coefficients' device")
    nb = i420_frame_bytes(W, H)
    if out is None:
        out = torch.empty(F_, nb, dtype=torch.uint8, device=coef.device)
    elif (out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != F_ or out.shape[1] < nb or out.stride(1) != 1
          or (F_ > 1 and out.stride(0) < nb) or out.device != coef.device):
        raise VFaceHipError(f"jpeg_planes: out must be uint8 [{F_}, >= {nb}] rows on the coefficients' device, unit column stride, "
                            f"row stride >= {nb}")
    cstride = coef.stride(0) if F_ > 1 else max(coef.stride(0), n)
    ostride = out.stride(0) if F_ > 1 else max(out.stride(0), nb)
    _check(load().vface_jpeg_planes(_p(coef), cstride, _p(quant), W, H, F_, _p(out), ostride, _stream()), "vface_jpeg_planes")
    return out


def quad_crop(frames: torch.Tensor, quads: torch.Tensor, windows: torch.Tensor, out_size: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``img.crop(window).transform((out_size, out_size), QUAD, .., BILINEAR)`` of uint8 frames [F, H, W, 3] (alignmengt.py:115-123,
    :142), bit-identical to Pillow.  ``quads`` float64 device [F, 8]: Pillow's QUAD coefficients in window coordinates;
    ``windows`` int32 [F, 4] (host or device): the crop window (x0, y0, x1, y1) of each frame, inside it and not empty.  Returns
    uint8 [F, out_size, out_size, 3] (``out`` if given)."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise VFaceHipError("quad_crop: frames must be contiguous uint8 [F, H, W, 3]")
    F_, H, W, _ = frames.shape
    if out_size <= 0 or F_ <= 0:
        raise VFaceHipError("quad_crop: the output size and the number of frames must be positive")
    if not quads.is_cuda or quads.dtype != torch.float64 or tuple(quads.shape) != (F_, 8) or not quads.is_contiguous():
        raise VFaceHipError("quad_crop: quads must be a contiguous float64 device tensor [F, 8]")
    if windows.dtype != torch.int32 or tuple(windows.shape) != (F_, 4):
        raise VFaceHipError("quad_crop: windows must be int32 [F, 4]")
    wh = windows.cpu()
    if bool(((wh[:, 0] < 0) | (wh[:, 1] < 0) | (wh[:, 2] > W) | (wh[:, 3] > H) | (wh[:, 0] >= wh[:, 2]) | (wh[:, 1] >= wh[:, 3])).any()):
        raise VFaceHipError("quad_crop: every window must be a non-empty rectangle inside its frame")
    windows = windows.to(frames.device).contiguous()
    if out is None:
        out = torch.empty(F_, out_size, out_size, 3, dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F_, out_size, out_size, 3) or not out.is_contiguous():
        raise VFaceHipError("quad_crop: out must be contiguous uint8 [F, out_size, out_size, 3]")
    rc = load().vface_quad_crop(_p(frames), W, H, _p(out), out_size, F_, _p(quads), _p(windows), _stream())
    _check(rc, "vface_quad_crop")
    return out


def label_membership(remove_labels, device) -> torch.Tensor:
    """The 256-entry table ``member[v] = v in remove_labels`` that ``dataset_tensors`` reads in place of ``np.isin``."""
    member = torch.zeros(256, dtype=torch.uint8)
    for v in remove_labels:
        if not 0 <= int(v) <= 255:
            raise VFaceHipError(f"label {v} is outside an 8-bit label map")
        member[int(v)] = 1
    return member.to(device)


def dataset_tensors(crop: torch.Tensor, label: torch.Tensor, member: torch.Tensor, latent: Tuple[int, int], out=None):
    """``VideoDataset.__getitem_gray__`` (video_swap_dataset.py:157-163, :214-221) + the mask resize of VFace_inference_batch.py:459
    for uint8 crops [F, H, W, 3] and uint8 label maps [F, H, W]; ``member``: ``label_membership(remove_labels)``; ``latent`` =
    (h, w) of the latent grid.  Returns fp32 ``image [F, 3, H, W], inpaint_image [F, 3, H, W], inpaint_mask [F, 1, H, W],
    mask_latent [F, 1, h, w]`` (written into the four tensors of ``out`` if given)."""
    if crop.dtype != torch.uint8 or crop.dim() != 4 or crop.shape[3] != 3 or not crop.is_contiguous():
        raise VFaceHipError("dataset_tensors: crops must be contiguous uint8 [F, H, W, 3]")
    F_, H, W, _ = crop.shape
    if label.dtype != torch.uint8 or tuple(label.shape) != (F_, H, W) or not label.is_contiguous():
        raise VFaceHipError(f"dataset_tensors: label maps must be contiguous uint8 {[F_, H, W]}, the crops' size; got {list(label.shape)}")
    if member.dtype != torch.uint8 or tuple(member.shape) != (256,) or not member.is_contiguous():
        raise VFaceHipError("dataset_tensors: member must be the uint8 [256] table of label_membership()")
    oh, ow = int(latent[0]), int(latent[1])
    if min(F_, H, W, oh, ow) <= 0:
        raise VFaceHipError("dataset_tensors: F, H, W and the latent grid must be positive")
    shapes = [(F_, 3, H, W), (F_, 3, H, W), (F_, 1, H, W), (F_, 1, oh, ow)]
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=crop.device) for s in shapes)
    for t, s in zip(out, shapes):
        if t.dtype != torch.float32 or tuple(t.shape) != s or not t.is_contiguous():
            raise VFaceHipError(f"dataset_tensors: outputs must be contiguous fp32 {shapes}")
    image, inpaint, mask, mlat = out
    rc = load().vface_dataset_tensors(_p(crop), _p(label), _p(member), W, H, _p(image), _p(inpaint), _p(mask), _p(mlat), ow, oh, F_,
                                      _stream())
    _check(rc, "vface_dataset_tensors")
    return image, inpaint, mask, mlat


def source_tensors(crop: torch.Tensor, img: torch.Tensor, label: torch.Tensor, member: torch.Tensor, taps, latent: Tuple[int, int],
                   clip_size: int, out=None, clip_u8: Optional[torch.Tensor] = None):
    """The source image's tensors (VFace_inference_batch.py:324-355, :462, :468) in one launch: uint8 aligned crops [N, S, S, 3],
    the same crops after the Pillow-bilinear resize ``img`` [N, H, W, 3] (:350), uint8 label maps [N, H, W]; ``member``:
    ``label_membership(preserve_labels)``; ``taps`` = ``(xtap, xw, ytap, yw)``, the device tables of ``resample.linear_taps_u8(S,
    clip_size)`` (int32 [clip_size, 2] / int16 [clip_size, 2]); ``latent`` = (h, w).  Returns fp32 ``mask [N, 1, H, W], masked
    [N, 3, H, W], inpaint [N, 3, H, W], mask_latent [N, 1, h, w], clip_image [N, 3, clip_size, clip_size]`` (written into the five
    tensors of ``out`` if given); ``clip_u8`` uint8 [N, clip_size, clip_size, 3], if given, receives the 8-bit resize itself.  That
    resize is OpenCV's 11-bit fixed-point form as DESIGN §9 states it; parity with ``cv2.resize`` is not pinned."""
    if crop.dtype != torch.uint8 or crop.dim() != 4 or crop.shape[3] != 3 or crop.shape[1] != crop.shape[2] or not crop.is_contiguous():
        raise VFaceHipError("source_tensors: crops must be contiguous uint8 [N, S, S, 3]")
    N, S = crop.shape[0], crop.shape[1]
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[0] != N or img.shape[3] != 3 or not img.is_contiguous():
        raise VFaceHipError("source_tensors: img must be contiguous uint8 [N, H, W, 3], one per crop")
    H, W = img.shape[1], img.shape[2]
    if label.dtype != torch.uint8 or tuple(label.shape) != (N, H, W) or not label.is_contiguous():
        raise VFaceHipError(f"source_tensors: label maps must be contiguous uint8 {[N, H, W]}, img's size; got {list(label.shape)}")
    if member.dtype != torch.uint8 or tuple(member.shape) != (256,) or not member.is_contiguous():
        raise VFaceHipError("source_tensors: member must be the uint8 [256] table of label_membership()")
    oh, ow, oc = int(latent[0]), int(latent[1]), int(clip_size)
    if min(N, S, H, W, oh, ow, oc) <= 0:
        raise VFaceHipError("source_tensors: N, S, H, W, the latent grid and clip_size must be positive")
    xtap, xw, ytap, yw = taps
    for t, dt in ((xtap, torch.int32), (xw, torch.int16), (ytap, torch.int32), (yw, torch.int16)):
        if t.dtype != dt or tuple(t.shape) != (oc, 2) or not t.is_contiguous():
            raise VFaceHipError("source_tensors: taps must be int32 [clip_size, 2] / int16 [clip_size, 2] tables (linear_taps_u8)")
    shapes = [(N, 1, H, W), (N, 3, H, W), (N, 3, H, W), (N, 1, oh, ow), (N, 3, oc, oc)]
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=crop.device) for s in shapes)
    for t, s in zip(out, shapes):
        if t.dtype != torch.float32 or tuple(t.shape) != s or not t.is_contiguous():
            raise VFaceHipError(f"source_tensors: outputs must be contiguous fp32 {shapes}")
    if clip_u8 is not None and (clip_u8.dtype != torch.uint8 or tuple(clip_u8.shape) != (N, oc, oc, 3) or not clip_u8.is_contiguous()):
        raise VFaceHipError(f"source_tensors: clip_u8 must be contiguous uint8 {[N, oc, oc, 3]}")
    mask, masked, inpaint, mlat, clip_image = out
    rc = load().vface_source_tensors(_p(crop), S, _p(img), _p(label), _p(member), W, H, _p(xtap), _p(xw), _p(ytap), _p(yw), _p(mask),
                                     _p(masked), _p(inpaint), _p(mlat), ow, oh, _p(clip_image), _p(clip_u8), oc, N, _stream())
    _check(rc, "vface_source_tensors")
    return mask, masked, inpaint, mlat, clip_image


# ---- glue of the face-parsing network (csrc/parsing.hip; include/vface_hip.h "face parsing") ----
def parse_prefilter(crops: torch.Tensor, out: torch.Tensor, factor: int = 2):
    """uint8 crops [F, 2h, 2w, 3] -> ``out`` 16-bit [F*h*w, 8] (3 normalised channels, 5 zeros): ``FaceParser.preprocess_img``."""
    if crops.dtype != torch.uint8 or crops.dim() != 4 or crops.shape[3] != 3 or not crops.is_contiguous():
        raise VFaceHipError("parse_prefilter: crops must be contiguous uint8 [F, H, W, 3]")
    F_, H2, W2, _ = crops.shape
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[1] < 8 or out.shape[0] != F_ * (H2 // 2) * (W2 // 2):
        raise VFaceHipError(f"parse_prefilter: out must be a 16-bit [F*h*w, >= 8] view; got {tuple(out.shape)}")
    rc = load().vface_parse_prefilter(_p(crops), W2, H2, factor, _p(out), out.stride(0), F_, dtype_code(out.dtype), _stream())
    _check(rc, "vface_parse_prefilter")


def maxpool3x3s2(x: torch.Tensor, y: torch.Tensor, *, nimg: int, H: int, W: int, C_: int, ldx: Optional[int] = None,
                 ldy: Optional[int] = None):
    rc = load().vface_maxpool3x3s2(_p(x), ldx if ldx is not None else x.stride(0), nimg, H, W, C_, _p(y),
                                   ldy if ldy is not None else y.stride(0), dtype_code(x.dtype), _stream())
    _check(rc, "vface_maxpool3x3s2")


def channel_gate(x: torch.Tensor, g: torch.Tensor, y: torch.Tensor, *, M: int, hw: int, C_: int, rvec=None, rten=None,
                 add_x: bool = False, ldx: Optional[int] = None, ldy: Optional[int] = None, ldr: Optional[int] = None):
    """``y = x * g[image] + r`` with ``r`` one of nothing, ``rvec`` (fp32 per image), ``rten`` (16-bit tensor), ``x`` itself."""
    for t in (g, rvec):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1):
            raise VFaceHipError("channel_gate: g and rvec are 2-D fp32 views [nimg, C] with unit column stride")
    rc = load().vface_channel_gate(_p(x), ldx if ldx is not None else x.stride(0), _p(g), g.stride(0), _p(rvec),
                                   rvec.stride(0) if rvec is not None else 0, _p(rten),
                                   (ldr if ldr is not None else rten.stride(0)) if rten is not None else 0, int(add_x), _p(y),
                                   ldy if ldy is not None else y.stride(0), M, hw, C_, dtype_code(x.dtype), _stream())
    _check(rc, "vface_channel_gate")


def pooled_linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, nimg: int, N: int, K: int,
                  lda: int, sa: int = 1, act: int = 0):
    """``out[n, :N] = act(w[:N, :K] @ a[n] + bias)`` in fp32; ``a`` element (n, k) at ``a.data_ptr + 4 * (n * lda + k * sa)``."""
    for t in (a, w, bias, out):
        if t is not None and t.dtype != torch.float32:
            raise VFaceHipError("pooled_linear: every operand is fp32")
    if not w.is_contiguous() or tuple(w.shape) != (N, K) or (bias is not None and bias.numel() != N):
        raise VFaceHipError("pooled_linear: w must be contiguous [N, K] and bias [N]")
    if a.numel() < (nimg - 1) * lda + (K - 1) * sa + 1 or out.dim() != 2 or out.shape[0] < nimg:
        raise VFaceHipError("pooled_linear: a / out are too small for nimg rows")
    rc = load().vface_pooled_linear(_p(a), lda, sa, _p(w), _p(bias), _p(out), out.stride(0), nimg, N, K, act, _stream())
    _check(rc, "vface_pooled_linear")


def upsample_argmax_u8(logits: torch.Tensor, table: torch.Tensor, *, F: int, h: int, w: int, ncls: int, H: int, W: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 logits [F*h*w, ld] -> uint8 [F, H, W] = table[argmax over the first ``ncls`` columns of the bilinear
    (align_corners) upsampling]; ``table``: uint8 [32] on the device."""
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] != F * h * w:
        raise VFaceHipError(f"upsample_argmax_u8: logits must be an fp32 [F*h*w, ld] view; got {tuple(logits.shape)}")
    if table.dtype != torch.uint8 or tuple(table.shape) != (32,) or not table.is_contiguous():
        raise VFaceHipError("upsample_argmax_u8: table must be uint8 [32]")
    if logits.shape[1] < ncls:
        raise VFaceHipError("upsample_argmax_u8: fewer logit columns than classes")
    if out is None:
        out = torch.empty(F, H, W, dtype=torch.uint8, device=logits.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (F, H, W) or not out.is_contiguous():
        raise VFaceHipError("upsample_argmax_u8: out must be contiguous uint8 [F, H, W]")
    rc = load().vface_upsample_argmax_u8(_p(logits), logits.stride(0), F, h, w, ncls, _p(table), _p(out), H, W, _stream())
    _check(rc, "vface_upsample_argmax_u8")
    return out


def ffn_fused_supported(M: int, C_: int) -> bool:
    return bool(load().vface_ffn_fused_supported(M, C_))


def attn_out_ffn_fused(att: torch.Tensor, resid32: torch.Tensor, rowbias: Optional[torch.Tensor], wo_w1: torch.Tensor, bo: torch.Tensor,
                       gamma: torch.Tensor, beta: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor, b2: torch.Tensor,
                       out16: Optional[torch.Tensor], *, M: int, C_: int, rows_per_sample: int, out32: Optional[torch.Tensor] = None,
                       eps: float = 1e-5):
    """attn1's out-projection + attn2's row bias + residual, norm3 and the FeedForward in ONE launch (``vface_attn_out_ffn_fused``):
    ``out = ff(LayerNorm(t1)) + t1`` with ``t1 = att @ Wo^T + bo + rowbias[sample] + resid32`` never stored."""
    o = out16 if out16 is not None else out32
    rc = load().vface_attn_out_ffn_fused(_p(att), att.stride(0), _p(resid32), resid32.stride(0), _p(rowbias),
                                         rowbias.stride(0) if rowbias is not None else 0, rows_per_sample, _p(wo_w1), _p(bo), _p(gamma),
                                         _p(beta), eps, _p(b1), _p(w2p), _p(b2), _p(out16), out16.stride(0) if out16 is not None else 0,
                                         _p(out32), out32.stride(0) if out32 is not None else 0, M, C_, dtype_code(att.dtype), _stream())
    _check(rc, "vface_attn_out_ffn_fused")


def attn_out_ffn_proj_fused(att: torch.Tensor, resid32: torch.Tensor, rowbias: Optional[torch.Tensor], w_stream: torch.Tensor,
                            bo: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor, b2: torch.Tensor,
                            b_po: torch.Tensor, x_in: torch.Tensor, out16: Optional[torch.Tensor], out32: Optional[torch.Tensor],
                            colstats: Optional[torch.Tensor], *, M: int, C_: int, rows_per_sample: int, eps: float = 1e-5):
    """``attn_out_ffn_fused`` + the SpatialTransformer's ``proj_out`` + ``x_in`` (+ column statistics) in ONE launch
    (``vface_attn_out_ffn_proj_fused``); ``w_stream`` = ``packing.pack_attn_out_ffn(w_o, w1_geglu, w_proj_out)``."""
    rc = load().vface_attn_out_ffn_proj_fused(
        _p(att), att.stride(0), _p(resid32), resid32.stride(0), _p(rowbias), rowbias.stride(0) if rowbias is not None else 0,
        rows_per_sample, _p(w_stream), _p(bo), _p(gamma), _p(beta), eps, _p(b1), _p(w2p), _p(b2), _p(b_po), _p(x_in), x_in.stride(0),
        _p(out16), out16.stride(0) if out16 is not None else 0, _p(out32), out32.stride(0) if out32 is not None else 0,
        _p(colstats), colstats.stride(0) // 2 if colstats is not None else 0, M, C_, dtype_code(att.dtype), _stream())
    _check(rc, "vface_attn_out_ffn_proj_fused")


def linear_small_supported(M: int, N: int, K: int) -> bool:
    return bool(load().vface_linear_small_supported(M, N, K))


def linear_small(a: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, M: int, N: int, K: int,
                 silu: bool = False):
    """``out[:M, :N] = act(a[:M, :K] @ wt[:N, :K]^T + bias)`` on a handful of rows (``vface_linear_small``: the time-embedding chain);
    ``out``: 16-bit or fp32."""
    rc = load().vface_linear_small(_p(a), a.stride(0), _p(wt), wt.stride(0), _p(bias), _p(out),
                                   out.stride(0), int(out.dtype == torch.float32), int(silu), M, N, K, dtype_code(wt.dtype), _stream())
    _check(rc, "vface_linear_small")


def gn_silu_conv3x3_small(x: torch.Tensor, gn_ab: torch.Tensor, wt: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *,
                          nimg: int, H: int, W: int, cin: int, cout: int):
    """GroupNorm-apply + SiLU + conv3x3 to 3 / 4 channels in one launch (the UNet's ``out`` layer, ``vface_gn_silu_conv3x3_small``);
    ``x``: the fp32 carrier or the 16-bit copy ``[nimg*H*W, cin]``; ``out``: fp32 ``[nimg*H*W, >= cout]``."""
    rc = load().vface_gn_silu_conv3x3_small(_p(x), x.stride(0), int(x.dtype == torch.float32), _p(gn_ab), gn_ab.stride(0) // 2, _p(wt),
                                            _p(bias), _p(out), out.stride(0), nimg, H, W, cin, cout, dtype_code(wt.dtype), _stream())
    _check(rc, "vface_gn_silu_conv3x3_small")


def st_front_supported(M: int, C_: int, hw: int) -> bool:
    return bool(load().vface_st_front_supported(M, C_, hw))


def st_front(x32: torch.Tensor, gn_ab: torch.Tensor, wcat: torch.Tensor, b_in: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
             t0: torch.Tensor, qkv: torch.Tensor, *, M: int, C_: int, hw: int, NQ: int, rows_full: int, nq_lo: int = 0,
             ln: Optional[torch.Tensor] = None, eps: float = 1e-5):
    """GroupNorm-apply -> proj_in (-> ``t0`` fp32) -> LayerNorm -> attn1 projection (-> ``qkv`` 16-bit) in one launch
    (csrc/stfront.hip).  ``gn_ab``: ``groupnorm_coeffs_from_cols`` of the producer of ``x32``; ``wcat``: ``packing.pack_st_front``."""
    if x32.dtype != torch.float32 or t0.dtype != torch.float32 or gn_ab.dtype != torch.float32:
        raise VFaceHipError("st_front: x32, t0 and gn_ab are fp32")
    rc = load().vface_st_front(_p(x32), x32.stride(0), _p(gn_ab), gn_ab.stride(0) // 2, hw, _p(wcat), _p(b_in), _p(gamma), _p(beta), eps,
                               _p(t0), t0.stride(0), _p(qkv), qkv.stride(0), _p(ln) if ln is not None else None,
                               ln.stride(0) if ln is not None else 0, M, C_, NQ, rows_full, nq_lo, dtype_code(qkv.dtype), _stream())
    _check(rc, "vface_st_front")


def ffn_fused_width_supported(C_: int) -> bool:
    """Does the fused FeedForward take blocks of this width at all (any row count)?  128 rows = one workgroup's tokens."""
    return bool(load().vface_ffn_fused_supported(128, C_))


def ffn_fused(x32: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor,
              b2: torch.Tensor, out16: Optional[torch.Tensor], *, M: int, C_: int, out32: Optional[torch.Tensor] = None,
              eps: float = 1e-5):
    """``out = ff.net[2](GEGLU(ff.net[0](LayerNorm(x32)))) + x32`` in one launch (``vface_ffn_fused``); ``w1`` / ``b1`` in the GEGLU
    packing of ``packing.pack_geglu``, ``w2p`` from ``packing.pack_ffn_w2``."""
    if x32.dtype != torch.float32 or x32.dim() != 2 or x32.stride(1) != 1:
        raise VFaceHipError("ffn_fused: x32 must be a 2-D fp32 view with unit column stride")
    rc = load().vface_ffn_fused(_p(x32), x32.stride(0), _p(gamma), _p(beta), eps, _p(w1), _p(b1), _p(w2p), _p(b2), _p(out16),
                                out16.stride(0) if out16 is not None else 0, _p(out32),
                                out32.stride(0) if out32 is not None else 0, M, C_, dtype_code(w1.dtype), _stream())
    _check(rc, "vface_ffn_fused")


def timestep_embedding(t: torch.Tensor, out: torch.Tensor, dim: int):
    assert t.dtype == torch.int64
    rc = load().vface_timestep_embedding(_p(t), _p(out), t.numel(), dim, dtype_code(out.dtype), _stream())
    _check(rc, "vface_timestep_embedding")


def silu(x: torch.Tensor, out: torch.Tensor):
    rc = load().vface_silu(_p(x), _p(out), x.numel(), int(x.dtype == torch.float32), dtype_code(out.dtype), _stream())
    _check(rc, "vface_silu")


def cast_f32(x: torch.Tensor, out: torch.Tensor):
    assert x.dtype == torch.float32
    rc = load().vface_cast_f32(_p(x), _p(out), x.numel(), dtype_code(out.dtype), _stream())
    _check(rc, "vface_cast_f32")


def pack_unet_input(x, inv, inpaint, mask, out, *, F, h, w, cpad):
    rc = load().vface_pack_unet_input(_p(x), _p(inv), _p(inpaint), _p(mask), _p(out), F, h, w, cpad,
                                      dtype_code(out.dtype), _stream())
    _check(rc, "vface_pack_unet_input")


def nchw_to_nhwc(x: torch.Tensor, out: torch.Tensor, *, N: int, C_: int, hw: int, cpad: int):
    rc = load().vface_nchw_to_nhwc(_p(x), _p(out), N, C_, hw, cpad, dtype_code(out.dtype), _stream())
    _check(rc, "vface_nchw_to_nhwc")


def nhwc_to_nchw_f32(x: torch.Tensor, out: torch.Tensor, *, N: int, C_: int, hw: int, ldx: int):
    rc = load().vface_nhwc_to_nchw_f32(_p(x), ldx, _p(out), N, C_, hw, _stream())
    _check(rc, "vface_nhwc_to_nchw_f32")


def ddim_step(eps, x, inv, x_prev, *, F, C_, hw, lde, scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, pred_x0=None,
              x_prev_recon=None, noise=None, single_branch=False):
    """``single_branch``: False / 0 = eps is [uncond ; cond ; recon]; True / 1 = one unguided branch (inversion); 2 = [uncond ;
    cond] only (the sampler's recon third left out)."""
    rc = load().vface_ddim_step(_p(eps), lde, _p(x), _p(inv), _p(x_prev), _p(pred_x0), _p(x_prev_recon), F, C_, hw,
                                scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, _p(noise), int(single_branch),
                                _stream())
    _check(rc, "vface_ddim_step")


def copy2d(src, dst, *, rows, cols, ld_src, ld_dst):
    rc = load().vface_copy2d(_p(src), ld_src, _p(dst), ld_dst, rows, cols, dtype_code(src.dtype), _stream())
    _check(rc, "vface_copy2d")


def temporal_gauss(src, dst1, dst2, *, F, n, C_, ld_src, fs_src, ld_dst, fs_dst):
    rc = load().vface_temporal_gauss(_p(src), ld_src, fs_src, _p(dst1), _p(dst2), ld_dst, fs_dst, F, n, C_,
                                     dtype_code(src.dtype), _stream())
    _check(rc, "vface_temporal_gauss")


def adain_fusion(a, b, dst, *, rows, C_, lda, ldb, ldd):
    lib = load()
    ws = torch.empty(int(lib.vface_adain_workspace_bytes(rows, C_)), dtype=torch.uint8, device=a.device)
    rc = lib.vface_adain_fusion(_p(a), lda, _p(b), ldb, _p(dst), ldd, rows, C_, _p(ws), ws.numel(), dtype_code(a.dtype),
                                _stream())
    _check(rc, "vface_adain_fusion")


def temporal_gauss_halo(src, prev, next_, dst1, dst2, *, F, first, F_total, n, C_, ld_src, fs_src, ld_dst, fs_dst,
                        ld_halo=0, fs_halo=0):
    """``temporal_gauss`` on frames [first, first + F) of an F_total-frame clip; ``prev`` / ``next_``: the two frames before / after
    the shard (slab s at ``s * fs_halo``), None where the shard touches the clip's end."""
    rc = load().vface_temporal_gauss_halo(_p(src), ld_src, fs_src, _p(prev), _p(next_), ld_halo, fs_halo, _p(dst1), _p(dst2), ld_dst,
                                          fs_dst, F, first, F_total, n, C_, dtype_code(src.dtype), _stream())
    _check(rc, "vface_temporal_gauss_halo")


def adain_rows_workspace_bytes(rows: int, C_: int) -> int:
    return int(load().vface_adain_rows_workspace_bytes(rows, C_))


def adain_rows(a, b, partial, ws, *, rows, C_, lda, ldb):
    """Pass 1 of ``adain_fusion``: fused rows into ``ws`` (``adain_rows_workspace_bytes``), fp64 ``partial`` [rows][2]."""
    assert partial.dtype == torch.float64 and partial.is_contiguous()
    rc = load().vface_adain_rows(_p(a), lda, _p(b), ldb, rows, C_, _p(partial), _p(ws), ws.numel() * ws.element_size(),
                                 dtype_code(a.dtype), _stream())
    _check(rc, "vface_adain_rows")


def adain_reduce_scale(partial, ws, dst, *, partial_rows, rows, C_, ldd):
    """Pass 2: the global std over ``partial`` [partial_rows][2] (all ranks' rows, global order), then dst = fused / (std + 1e-5)."""
    assert partial.dtype == torch.float64 and partial.is_contiguous()
    rc = load().vface_adain_reduce_scale(_p(partial), partial_rows, C_, _p(ws), ws.numel() * ws.element_size(), _p(dst), ldd, rows,
                                         dtype_code(dst.dtype), _stream())
    _check(rc, "vface_adain_reduce_scale")


def softmax_rows(scores: torch.Tensor, out: torch.Tensor, *, M: int, N: int, scale: float, ld_s: Optional[int] = None,
                 ld_p: Optional[int] = None):
    """out[m, :N] = softmax(scores[m, :N] * scale); fp32 in, 16-bit out."""
    rc = load().vface_softmax_rows(_p(scores), ld_s if ld_s is not None else scores.stride(0), _p(out),
                                   ld_p if ld_p is not None else out.stride(0), M, N, scale, dtype_code(out.dtype), _stream())
    _check(rc, "vface_softmax_rows")


def vae_sample(moments: torch.Tensor, noise: Optional[torch.Tensor], z: torch.Tensor, *, F: int, hw: int, zc: int,
               scale: float):
    rc = load().vface_vae_sample(_p(moments), moments.stride(0), _p(noise), _p(z), F, hw, zc, scale, _stream())
    _check(rc, "vface_vae_sample")


def upsample2x_conv3x3(x: torch.Tensor, wt_phases: torch.Tensor, out: torch.Tensor, *, nimg: int, H: int, W: int, cin: int,
                       cout: int, ldx: int, ldy: int, bias=None, rowbias=None, flags: int = 0, colstats=None, out32=None):
    """conv3x3(nearest_upsample2x(x)) as four parity-phase 2x2 convolutions (4/9 of the multiply-adds).
    ``wt_phases``: [4, cout, 4*cin] from ``packing.pack_upsample_phases``; ``out``: [nimg*2H*2W, >= cout]."""
    lib = load()
    for py in (0, 1):
        for px in (0, 1):
            rc = lib.vface_upsample2x_conv3x3_phase(_p(x), ldx, nimg, H, W, cin, _p(wt_phases[2 * py + px]), 4 * cin, cout, py, px,
                                                    _p(bias), _p(rowbias), rowbias.stride(0) if rowbias is not None else 0,
                                                    _p(out), ldy, _p(zeros_page(x.device)), flags, dtype_code(x.dtype),
                                                    _p(colstats), colstats.stride(0) // 2 if colstats is not None else 0,
                                                    _stream(), _s32(None, out32))
            _check(rc, "vface_upsample2x_conv3x3_phase")


def conv3x3_plus_1x1(x: torch.Tensor, x2: torch.Tensor, wt: torch.Tensor, out: torch.Tensor, *, nimg: int, H: int, W: int,
                     cin: int, c2: int, cout: int, ldx: int, ldx2: int, ldy: int, bias=None, rowbias=None, flags: int = 0,
                     colstats=None, split_k: bool = True, out32=None, gn_ab=None, gn_silu: bool = False):
    """out = conv3x3(x) + x2 @ W2^T + bias (a ResBlock's second conv plus its 1x1 shortcut); ``wt``: [cout, 9*cin + c2]."""
    lib = load()
    M, K = nimg * H * W, 9 * cin + c2
    ws, ws_bytes = splitk_workspace(x.device, M, cout, K, flags, H * W) if split_k else (None, 0)
    rc = lib.vface_conv3x3_plus_1x1(_p(x), ldx, nimg, H, W, cin, _p(x2), ldx2, c2, _p(wt), K, cout, _p(bias), _p(rowbias),
                                    rowbias.stride(0) if rowbias is not None else 0, _p(out), ldy, _p(zeros_page(x.device)),
                                    flags, dtype_code(x.dtype), _p(colstats),
                                    colstats.stride(0) // 2 if colstats is not None else 0, _p(ws), ws_bytes, _stream(),
                                    _s32(None, out32, gn_ab, gn_silu))
    _check(rc, "vface_conv3x3_plus_1x1")


# ---------------------------------------------------------------------------------------------- conditioning (csrc/clip.hip)
CLIP_PATCH, CLIP_PATCH_K, CLIP_PATCH_KP = 14, 588, 640      # the patch convolution's window, its K = 3 * 14 * 14 and K padded to 64
ACT_QUICK_GELU, ACT_GELU_ERF = 0, 1


def clip_patches(img: torch.Tensor, out: torch.Tensor, *, B: int, grid: int, H: int, W: int, ldo: int, prep: bool, mask=None,
                 dbg_x0=None, dbg_y0=None):
    """``img`` fp32 planar [B, 3, H, W] -> the patch matrix ``out`` [B grid grid, >= 640] (16-bit), column c 196 + ky 14 + kx, zero
    from 588 on.  ``prep``: un_norm + CLIP normalise + bilinear resize to 14 grid (``mask`` fp32 [B, H, W]: times (1 - mask) first);
    otherwise a copy of an already normalised 14 grid x 14 grid image."""
    for t in (img, mask):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise VFaceHipError("clip_patches: img / mask must be contiguous fp32")
    for t in (dbg_x0, dbg_y0):
        if t is not None and (t.dtype != torch.int32 or t.numel() < CLIP_PATCH * grid):
            raise VFaceHipError("clip_patches: dbg_x0 / dbg_y0 must be int32 [14 grid]")
    rc = load().vface_clip_patches(_p(img), H, W, _p(mask), int(prep), _p(out), ldo, B, grid, _p(dbg_x0), _p(dbg_y0),
                                   dtype_code(out.dtype), _stream())
    _check(rc, "vface_clip_patches")


def clip_embed(tok: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, x32: torch.Tensor, *, B: int, patches: int, C_: int, ldt: int,
               ldo: int, gamma=None, beta=None, eps: float = 1e-5):
    """x32 [B (patches + 1), C] fp32 = the class row and the patch rows ``tok`` (16-bit or fp32) plus the position table; with
    ``gamma`` / ``beta`` (fp32 [C]) the LayerNorm of those rows (``pre_layrnorm``)."""
    f32 = tok.dtype == torch.float32
    for t in (cls, pos, x32, gamma, beta):
        if t is not None and t.dtype != torch.float32:
            raise VFaceHipError("clip_embed: cls, pos, gamma, beta and x32 must be fp32")
    if not pos.is_contiguous():
        raise VFaceHipError("clip_embed: pos must be contiguous [patches + 1, C]")
    rc = load().vface_clip_embed(_p(tok), ldt, int(f32), _p(cls), _p(pos), _p(gamma), _p(beta), eps, _p(x32), ldo, B, patches, C_,
                                 F16 if f32 else dtype_code(tok.dtype), _stream())
    _check(rc, "vface_clip_embed")


def act(x: torch.Tensor, y: torch.Tensor, *, rows: int, cols: int, ldx: int, ldy: int, kind: int):
    """y = quick_gelu(x) (``ACT_QUICK_GELU``) or erf-GELU(x) (``ACT_GELU_ERF``) on 16-bit [rows, cols] views; ``y`` may be ``x``."""
    rc = load().vface_act(_p(x), ldx, _p(y), ldy, rows, cols, kind, dtype_code(x.dtype), _stream())
    _check(rc, "vface_act")


def cond_mix(operands, *, B: int, N: int, out32=None, out16=None, ldo32: int = 0, ldo16: int = 0, w_sum: Optional[float] = None):
    """``operands``: three ``(tensor | None, weight)`` pairs, each tensor contiguous fp32 [B, N] or [1, N] (one row for every sample):
    out = (a w_a + b w_b + c w_c) / w_sum, ``w_sum`` defaulting to the sum of the weights of the operands present."""
    assert len(operands) == 3
    args = []
    for t, w in operands:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() % N):
            raise VFaceHipError("cond_mix: operands must be contiguous fp32 [B | 1, N]")
        args += [_p(t), t.numel() // N if t is not None else 0, float(w)]
    if w_sum is None:
        w_sum = sum(float(w) for t, w in operands if t is not None)
    rc = load().vface_cond_mix(*args, float(w_sum), _p(out32), ldo32, _p(out16), ldo16, B, N,
                               dtype_code(out16.dtype) if out16 is not None else F16, _stream())
    _check(rc, "vface_cond_mix")


# ---- glue of the identity network (csrc/arcface.hip; include/vface_hip.h "identity features") ----
ID_SIZE = 112                 # the network's input, after the pooling and crop chain of ``extract_feats``


def id_prep(img: torch.Tensor, out: torch.Tensor, *, clip_img: bool = True, prep: bool = False, mask=None):
    """``img`` fp32 planar [B, 3, H, W] -> ``out`` 16-bit [B 112 112, >= 8] (3 values, 5 zeros): ``IDLoss.extract_feats`` up to the
    network.  ``prep``: ``img`` is a [-1, 1] frame (``mask`` fp32 [B, H, W]: times (1 - mask) first), brought to the CLIP image as
    ``clip_patches(prep=True)`` does."""
    for t in (img, mask):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise VFaceHipError("id_prep: img / mask must be contiguous fp32")
    if img.dim() != 4 or img.shape[1] != 3:
        raise VFaceHipError(f"id_prep: img must be [B, 3, H, W]; got {tuple(img.shape)}")
    B, _, H, W = img.shape
    if mask is not None and mask.numel() != B * H * W:
        raise VFaceHipError("id_prep: mask must be [B, H, W]")
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[1] < 8 or out.shape[0] != B * ID_SIZE * ID_SIZE:
        raise VFaceHipError(f"id_prep: out must be a 16-bit [B*112*112, >= 8] view; got {tuple(out.shape)}")
    rc = load().vface_id_prep(_p(img), H, W, _p(mask), int(prep), int(clip_img), _p(out), out.stride(0), B, dtype_code(out.dtype),
                              _stream())
    _check(rc, "vface_id_prep")


def _zargs(z, za, zb, C_: int, what: str):
    if z is None:
        return None, None, None, 0
    for t in (za, zb):
        if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C_:
            raise VFaceHipError(f"{what}: with z, za and zb are contiguous fp32 [C]")
    return _p(za), _p(zb), _p(z), z.stride(0)


def prelu(x: torch.Tensor, slope: torch.Tensor, y: torch.Tensor, *, M: int, C_: int, z=None, za=None, zb=None,
          ldx: Optional[int] = None, ldy: Optional[int] = None):
    """``y = x > 0 ? x : slope[c] x`` on 16-bit views (``y`` may be ``x``); ``z = za[c] y32 + zb[c]`` if given."""
    if slope.dtype != torch.float32 or not slope.is_contiguous() or slope.numel() != C_:
        raise VFaceHipError("prelu: slope must be contiguous fp32 [C]")
    pa, pb, pz, ldz = _zargs(z, za, zb, C_, "prelu")
    rc = load().vface_prelu(_p(x), ldx if ldx is not None else x.stride(0), _p(slope), _p(y), ldy if ldy is not None else y.stride(0),
                            pa, pb, pz, ldz, M, C_, dtype_code(x.dtype), _stream())
    _check(rc, "vface_prelu")


def se_gate_add(res: torch.Tensor, g: torch.Tensor, sc: torch.Tensor, y: torch.Tensor, *, nimg: int, H: int, W: int, C_: int,
                sc_stride: int = 0, z=None, za=None, zb=None):
    """``y = res * g[image] + shortcut``: ``sc_stride == 0`` reads row m of ``sc`` (the output's size, H x W); 1 | 2 reads pixel
    (oy s, ox s) of the unit's H x W input ``sc``.  ``z = za[c] y32 + zb[c]`` if given."""
    if g.dtype != torch.float32 or g.dim() != 2 or g.stride(1) != 1 or g.shape[0] < nimg:
        raise VFaceHipError("se_gate_add: g is a 2-D fp32 view [nimg, C] with unit column stride")
    pa, pb, pz, ldz = _zargs(z, za, zb, C_, "se_gate_add")
    rc = load().vface_se_gate_add(_p(res), res.stride(0), _p(g), g.stride(0), _p(sc), sc.stride(0), sc_stride, nimg, H, W, C_, _p(y),
                                  y.stride(0), pa, pb, pz, ldz, dtype_code(res.dtype), _stream())
    _check(rc, "vface_se_gate_add")


def l2norm_rows(x: torch.Tensor, out: torch.Tensor, *, B: int, N: int):
    """``out[b] = x[b] / ||x[b]||_2`` on fp32 2-D views with unit column stride."""
    for t in (x, out):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < B or t.shape[1] < N:
            raise VFaceHipError("l2norm_rows: x and out are fp32 [>= B, >= N] views with unit column stride")
    rc = load().vface_l2norm_rows(_p(x), x.stride(0), _p(out), out.stride(0), B, N, _stream())
    _check(rc, "vface_l2norm_rows")
