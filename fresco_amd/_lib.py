"""ctypes binding of libfresco_hip.so (the C ABI declared in include/fresco_hip.h).

The product path has no CPU or PyTorch-eager fallback: if the shared library is missing or does not
load, every operator of this package raises (``FrescoHipError``) instead of computing elsewhere.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FRESCO_HIP_LIB: an alternative build of the same library (A/B measurements of kernel variants, tools/ab_variants.sh);
# it must exist and export every symbol like the default one -- there is no fallback either way
LIB_PATH = os.environ.get("FRESCO_HIP_LIB") or os.path.join(_HERE, "lib", "libfresco_hip.so")

OK = 0
ERRORS = {
    -1: "FRESCO_EINVAL (null pointer / bad size / inconsistent arguments)",
    -2: "FRESCO_EUNSUPPORTED (shape outside what the kernels are built for)",
    -3: "FRESCO_EWORKSPACE (workspace too small)",
    -4: "FRESCO_ELAUNCH (HIP launch failed)",
}
F16, F32, BF16 = 0, 1, 2
# what fresco_version() of the library these SIGNATURES describe reports: an older build exports the same names with other
# argument lists
VERSION = "0.5.0.4"  # (0.5.0.2: the fresco_egnet_* and fresco_canny_* entry points moved into this library; 0.5.0.3: unet_*;
# 0.5.0.4: unet_layernorm and unet_geglu)


class FrescoHipError(RuntimeError):
    pass


_c = ctypes
_vp, _i, _f, _d, _sz, _i64 = _c.c_void_p, _c.c_int, _c.c_float, _c.c_double, _c.c_size_t, _c.c_int64

# name -> (restype, argtypes); must list every symbol include/fresco_hip.h declares
SIGNATURES = {
    "fresco_version": (_c.c_char_p, []),
    "fresco_last_error": (_c.c_char_p, []),
    "fresco_prof_enable": (_i, [_i]),
    "fresco_prof_disable": (_i, []),
    "fresco_prof_read": (_i, [_i, _vp, _vp, _vp]),
    "fresco_attn_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fresco_attn_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i64, _f, _f, _i64, _i64, _i, _vp]),
    "fresco_attn_kvproj_supported": (_i, [_i, _i, _i]),
    "fresco_attn_fwd_kvproj": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _f, _i64, _i,
                                    _vp]),
    "fresco_temporal_attn": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i64, _i64, _i64, _i, _vp]),
    "fresco_temporal_pack": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i64, _i64, _i64, _vp]),
    "fresco_temporal_attn_packed": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "fresco_temporal_unpack": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "fresco_flow_warp": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "fresco_resize_bilinear": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp]),
    "fresco_max_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "fresco_dilate": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "fresco_linear": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i, _i,
                           _i, _i, _i, _vp]),
    "fresco_linear_plan": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "fresco_attn_f32_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fresco_attn_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "fresco_fn_gemm": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64] + [_i] * 4 + [_f, _f] + [_i] * 8 + [_vp, _vp, _vp, _vp, _vp, _i, _i64, _vp]),
    "fresco_fn_colstats_finish": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "fresco_fn_colstats_workspace_bytes": (_sz, [_i, _i, _i]),
    "fresco_fn_colstats": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _f, _vp]),
    "fresco_fn_prep": (_i, [_vp] * 7 + [_i64, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "fresco_fn_layernorm": (_i, [_vp] * 7 + [_i64, _i64, _i64, _i, _f, _f, _vp, _vp]),
    "fresco_fn_conv7_rgb": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "fresco_fn_convex_upsample": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "fresco_flow_occlusion": (_i, [_vp] * 5 + [_i, _i, _i, _i, _f, _f, _f, _vp]),
    "fresco_warp_fuse_chain": (_i, [_vp] * 8 + [_i, _i, _i, _i, _i, _vp]),
    "fresco_adain": (_i, [_vp, _vp, _vp, _i, _i, _f, _f, _i, _vp]),
    "fresco_chan_mean_std": (_i, [_vp, _vp, _vp, _i, _i, _f, _i, _vp]),
    "fresco_opt_workspace_bytes": (_sz, [_i] * 7),
    "fresco_ctx_create": (_i, [_vp]),
    "fresco_ctx_destroy": (_i, [_vp]),
    "fresco_opt_run": (_i, [_vp] * 8 + [_sz, _i, _i, _i, _i, _i, _f, _i, _f, _f, _f, _f, _vp]),
    "fresco_opt_loss_grad": (_i, [_vp] * 9 + [_sz, _i, _i, _i, _i, _i, _f, _vp]),
    "fresco_opt_sharded_workspace_bytes": (_sz, [_i] * 7),
    "fresco_opt_sharded_begin": (_i, [_vp] * 5 + [_sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "fresco_opt_sharded_step": (_i, [_vp] * 9 + [_sz, _i, _i, _i, _i, _i, _i, _f, _i, _f, _f, _f, _f, _i, _vp]),
    "fresco_mapping_workspace_bytes": (_sz, [_i, _i, _i]),
    "fresco_mapping_ind": (_i, [_vp] * 7 + [_sz, _i, _i, _i, _f, _vp]),
    "fresco_ddpm_x0": (_i, [_vp] * 5 + [_i64, _f, _f, _f, _i, _vp]),
    "fresco_ddpm_prev": (_i, [_vp] * 4 + [_i64, _i64, _f, _f, _f, _i, _vp]),
    "fresco_gram_target_workspace_bytes": (_sz, [_i, _i, _i]),
    "fresco_gram_target": (_i, [_vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "fresco_ebsynth_max_levels": (_i, [_i] * 5),
    "fresco_ebsynth_workspace_bytes": (_sz, [_i] * 9),
    "fresco_ebsynth_run": (_i, [_vp] * 6 + [_i] * 6 + [_f, _i, _i, _i, _vp, _vp, _vp, _i, _c.c_uint64, _vp, _vp, _vp,
                                                     _vp, _sz, _vp]),
    "fresco_ebsynth_batch_workspace_bytes": (_sz, [_i] * 10),
    "fresco_ebsynth_run_batch": (_i, [_i] + [_vp] * 6 + [_i] * 6 + [_f, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                                                              _vp, _vp, _sz, _vp]),
    "fresco_ebsynth_stage_workspace_bytes": (_sz, [_i] * 4),
    "fresco_ebsynth_resample": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _sz, _vp]),
    "fresco_ebsynth_stop_mask": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "fresco_edge_guide": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "fresco_warp_nearest": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "fresco_blend_workspace_bytes": (_sz, [_i, _i]),
    "fresco_blend_frame": (_i, [_vp] * 4 + [_i, _i, _d, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fresco_bgr_to_lab_u8": (_i, [_vp, _vp, _i, _vp]),
    "fresco_lab_to_bgr_u8": (_i, [_vp, _vp, _i, _vp]),
    "fresco_histogram_blend": (_i, [_vp] * 3 + [_i, _i, _d, _d, _vp, _vp, _vp, _sz, _vp]),
    "fresco_poisson_fusion": (_i, [_vp] * 4 + [_i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fresco_flowcalc_input": (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    "fresco_flowcalc_output": (_i, [_vp] * 5 + [_i, _i, _i, _f, _f, _vp]),
    "fresco_freeu_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fresco_freeu_fourier": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _f, _i, _vp]),
    "fresco_freeu_backbone": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _i, _f, _vp, _sz, _i, _vp]),
    "fresco_hed_input": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "fresco_hed_side_pool": (_i, [_vp] * 6 + [_i, _i, _i, _i, _f, _vp, _vp]),
    "fresco_hed_fuse": (_i, [_vp] * 8 + [_i, _i, _i, _i, _vp]),
    "fresco_egnet_input": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "fresco_egnet_pool": (_i, [_vp] * 4 + [_i, _i, _i, _i, _f, _vp, _vp]),
    "fresco_egnet_resize_add": (_i, [_vp] * 5 + [_i] * 7 + [_f, _vp, _vp]),
    "fresco_egnet_saliency": (_i, [_vp, _vp, _vp] + [_i] * 6 + [_vp]),
    "fresco_canny_workspace_bytes": (_sz, [_i, _i, _i]),
    "fresco_canny_classify": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "fresco_canny_hysteresis": (_i, [_vp, _vp, _vp, _i, _vp, _sz, _i, _i, _i, _vp]),
}

# the key-frame selection kernels (csrc/keyframe.hip) in the same library, declared in include/fresco_keyframe.h: named
# keyframe_*, beside the fresco_* surface that SIGNATURES and include/fresco_hip.h describe; bound on the same handle
KEYFRAME_SIGNATURES = {
    "keyframe_resize_table_bytes": (_sz, [_i, _i, _i, _i]),
    "keyframe_resize_table": (_i, [_i, _i, _i, _i, _vp, _sz]),
    "keyframe_resize_area_u8": (_i, [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "keyframe_workspace_bytes": (_sz, [_i, _i, _i]),
    "keyframe_frame_errors": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
}

# the tap resizes (csrc/resize.hip: INTER_LANCZOS4, and INTER_AREA's rule where a side is enlarged), declared in
# include/fresco_resize.h: named frame_resize_*, beside both pinned surfaces; bound on the same handle
RESIZE_SIGNATURES = {
    "frame_resize_table_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "frame_resize_table": (_i, [_i, _i, _i, _i, _i, _vp, _sz]),
    "frame_resize_u8": (_i, [_vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp]),
}
RESIZE_LANCZOS4, RESIZE_LINEAR_AREA = 0, 1  # FRAME_RESIZE_* of the header

# the MiDaS depth annotator's kernels (csrc/midas.hip, and the stem's "same" origin in csrc/flownet.hip), declared in
# include/fresco_midas.h: named midas_*, beside the pinned surfaces; bound on the same handle
MIDAS_SIGNATURES = {
    "midas_input": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "midas_stem_conv": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "midas_groupnorm_workspace_bytes": (_sz, [_i, _i, _i]),
    "midas_groupnorm_stats": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _f, _vp]),
    "midas_groupnorm_apply": (_i, [_vp] * 9 + [_i] * 7 + [_f, _vp, _vp]),
    "midas_pool": (_i, [_vp] * 4 + [_i, _i, _i, _i, _f, _vp, _vp]),
    "midas_layernorm": (_i, [_vp] * 6 + [_i64, _i, _f, _f, _vp, _vp]),
    "midas_tokens": (_i, [_vp] * 4 + [_i, _i, _i, _vp]),
    "midas_head_merge": (_i, [_vp] * 4 + [_i, _i, _i, _f, _vp, _vp]),
    "midas_rowbias_gelu": (_i, [_vp] * 5 + [_i64, _i, _i, _f, _vp, _vp]),
    "midas_tail_workspace_bytes": (_sz, [_i, _i, _i]),
    "midas_tail": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _sz, _i, _i, _i, _f, _f, _vp]),
}

# the VAE decoder's kernels (csrc/vae.hip), declared in include/fresco_vae.h: named vae_*, beside the pinned surfaces; bound
# on the same handle
VAE_SIGNATURES = {
    "vae_input": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "vae_conv": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp] + [_i] * 9 + [_i64, _vp]),
    "vae_groupnorm_workspace_bytes": (_sz, [_i, _i, _i]),
    "vae_groupnorm": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _f, _i, _vp]),
    "vae_softmax": (_i, [_vp, _vp, _i64, _i, _i64, _i64, _f, _vp]),
}
VAE_OUT_F16, VAE_OUT_F32, VAE_OUT_F16_NCHW = 0, 1, 2  # VAE_OUT_* of the header
# VAE_ELEM_BF16 (OR-ed into vae_conv's out_kind) = UNET_ELEM_BF16 (into unet_groupnorm's silu word): bf16 operands
ELEM_BF16 = 0x100

# what the VAE encoder adds to them (csrc/vae_enc.hip), declared in include/fresco_vae_enc.h: named vaeenc_*
VAE_ENC_SIGNATURES = {
    "vaeenc_input": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "vaeenc_conv_down": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "vaeenc_moments": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "vaeenc_sample": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp]),
}

# the UNet resnet block's kernels (csrc/unet.hip), declared in include/fresco_unet.h: named unet_*
UNET_SIGNATURES = {
    "unet_groupnorm_workspace_bytes": (_sz, [_i, _i, _i]),
    "unet_groupnorm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _f, _i, _vp]),
    "unet_groupnorm_lds_form": (_i, [_i, _i, _i]),
    "unet_temb": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "unet_temb_dt": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),   # + dtype: F16 or BF16
}

# what the UNet transformer blocks add to them (csrc/unet_tf.hip), declared in include/fresco_unet_tf.h: named unet_* too
UNET_TF_SIGNATURES = {
    "unet_layernorm": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i, _f, _vp]),
    "unet_geglu": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i64, _vp]),
}

# flash attention at head dim 160 for the plain attention processor (csrc/unet_attn.hip), declared in
# include/fresco_unet_attn.h: named unet_* too
UNET_ATTN_SIGNATURES = {
    "unet_attention": (_i, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _i, _f, _i, _vp]),
}

# what is left of the UNet and the ControlNet around those (csrc/unet_shell.hip), declared in include/fresco_unet_shell.h:
# named unet_* too
UNET_SHELL_SIGNATURES = {
    "unet_conv3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "unet_input": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "unet_time_linear": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
}
UNET_ACT_NONE, UNET_ACT_SILU = 0, 1            # UNET_ACT_* of the header
UNET_SRC_TIMESTEPS, UNET_SRC_SILU_ROWS = 0, 1  # UNET_SRC_* of the header

# the CLIP text model's kernels (csrc/text.hip), declared in include/fresco_text.h: named clip_*, beside the pinned surfaces;
# bound on the same handle
TEXT_SIGNATURES = {
    "clip_embed": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "clip_attention": (_i, [_vp, _vp, _vp, _i64, _vp, _i64, _i, _i, _i, _i, _f, _i, _vp]),
    "clip_fc1": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i64, _vp]),
}

# the denoising loop's glue (csrc/loop.hip), declared in include/fresco_loop.h: named loop_*, beside the pinned surfaces; bound
# on the same handle.  The version string did not move for them: a library built before them is refused because it does not
# export them, and the error names the symbol
LOOP_SIGNATURES = {
    "loop_update": (_i, [_vp] * 8 + [_i, _i64, _i64, _i64, _i] + [_f] * 6 + [_i, _vp]),
    "loop_image_to_frames": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
}

_lib = None


def load():
    """Load the library (once) and return the ctypes handle; raises FrescoHipError if it cannot."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FrescoHipError(
            "fresco_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C fresco_amd/csrc`. There is no CPU / eager fallback." % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise FrescoHipError("fresco_amd: cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in list(SIGNATURES.items()) + list(KEYFRAME_SIGNATURES.items()) + list(RESIZE_SIGNATURES.items()) \
            + list(MIDAS_SIGNATURES.items()) + list(VAE_SIGNATURES.items()) + list(VAE_ENC_SIGNATURES.items()) + list(UNET_SIGNATURES.items()) \
            + list(UNET_TF_SIGNATURES.items()) + list(UNET_ATTN_SIGNATURES.items()) + list(UNET_SHELL_SIGNATURES.items()) \
            + list(TEXT_SIGNATURES.items()) + list(LOOP_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise FrescoHipError("fresco_amd: %s does not export %s (stale build?)" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    built = lib.fresco_version().decode().split()
    if built[1:2] != [VERSION]:
        raise FrescoHipError("fresco_amd: %s is version %s, this package binds %s (stale build?)"
                             % (LIB_PATH, " ".join(built[1:2]) or "?", VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != OK:
        detail = ""
        if rc == -4:
            detail = ": " + load().fresco_last_error().decode()
        raise FrescoHipError("%s failed: %s%s" % (what, ERRORS.get(rc, "error %d" % rc), detail))
