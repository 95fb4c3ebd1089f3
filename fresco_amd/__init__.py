"""fresco_amd -- MI355X-native (gfx950) implementation of FRESCO's hot path: flow-guided spatial /
cross-frame / temporal attention, bilinear feature warp + fuse, and the feature-optimisation loop,
behind the reference's own plugin surface (diffusers AttnProcessor + UNet forward hook).

Everything computes in libfresco_hip.so (hand-written HIP, C ABI in include/fresco_hip.h); importing
the package does not need a GPU, calling any operator does, and there is no CPU fallback.
"""
from ._lib import FrescoHipError, LIB_PATH
from .control import AttentionControl
from .processor import FRESCOAttnProcessor2_0, apply_FRESCO_attn
from .opt import optimize_feature
from .warp import Dilate, adaptive_instance_normalization, calc_mean_std, flow_warp, warp_tensor
from .hook import apply_FRESCO_opt, disable_FRESCO_opt, patch_reference
from .mapping import cross_frame_masks, get_mapping_ind, get_single_mapping_ind
from .step import predict_x0, step
from .loop import inference, tensor2numpy
from .ebsynth import ebsynth_run, ebsynth_run_batch
from . import blend
from .flowcalc import FlowCalc, patch_flow_calc
from .freeu import (Fourier_filter, apply_freeu, patch_free_lunch, register_free_crossattn_upblock2d,
                    register_free_upblock2d)
from .hed import ControlNetHED_Apache2, DoubleConvBlock, HEDdetector, patch_hed
from .egnet import TUN_bone, build_model, get_saliency, patch_saliency
from .canny import CannyDetector, patch_canny
from .midas import DPTDepthModel, MidasDetector, patch_midas
from .vae import (VAEDecoder, VAEEncoder, patch_vae, patch_vae_decode, patch_vae_encode, unpatch_vae, unpatch_vae_decode,
                  unpatch_vae_encode)
from .unet_resnet import UNetResnet, patch_unet_resnets, unpatch_unet_resnets
from .unet_transformer import UNetTransformer, patch_unet_transformers, unpatch_unet_transformers
from .unet_attention import UNetAttnProcessor, patch_unet_attention, unpatch_unet_attention
from .unet_shell import (ControlNetCondEmbedding, UNetConvIn, UNetConvOut, UNetDownsample, UNetTimeEmbedding, UNetUpsample,
                         UNetZeroConv, patch_unet_shell, unpatch_unet_shell)
from .text_encoder import CLIPTextEncoder, patch_text_encoder, unpatch_text_encoder
from .keyframe import (frame_errors, get_keyframe_ind, patch_keyframe_selection, resize_frames, resize_image, resize_size,
                       select_keyframes)
from .paras import (correlation_matrices, forward_backward_consistency_check, get_flow_and_interframe_paras,
                    get_intraframe_paras, interframe_paras_from_flows)

__all__ = [
    "AttentionControl", "FRESCOAttnProcessor2_0", "apply_FRESCO_attn", "optimize_feature",
    "warp_tensor", "flow_warp", "adaptive_instance_normalization", "calc_mean_std", "Dilate", "apply_FRESCO_opt",
    "disable_FRESCO_opt", "patch_reference", "get_mapping_ind", "get_single_mapping_ind", "cross_frame_masks",
    "step", "predict_x0", "inference", "tensor2numpy", "get_flow_and_interframe_paras", "get_intraframe_paras", "interframe_paras_from_flows",
    "forward_backward_consistency_check", "correlation_matrices",
    "ebsynth_run", "ebsynth_run_batch", "blend", "FlowCalc", "patch_flow_calc", "FrescoHipError", "LIB_PATH",
    "Fourier_filter", "register_free_upblock2d", "register_free_crossattn_upblock2d", "apply_freeu", "patch_free_lunch",
    "HEDdetector", "ControlNetHED_Apache2", "DoubleConvBlock", "patch_hed",
    "TUN_bone", "build_model", "get_saliency", "patch_saliency",
    "CannyDetector", "patch_canny",
    "MidasDetector", "DPTDepthModel", "patch_midas",
    "VAEDecoder", "patch_vae_decode", "unpatch_vae_decode",
    "VAEEncoder", "patch_vae_encode", "unpatch_vae_encode", "patch_vae", "unpatch_vae",
    "UNetResnet", "patch_unet_resnets", "unpatch_unet_resnets",
    "UNetTransformer", "patch_unet_transformers", "unpatch_unet_transformers",
    "UNetAttnProcessor", "patch_unet_attention", "unpatch_unet_attention",
    "UNetDownsample", "UNetUpsample", "UNetConvIn", "UNetConvOut", "UNetTimeEmbedding", "ControlNetCondEmbedding",
    "UNetZeroConv", "patch_unet_shell", "unpatch_unet_shell",
    "CLIPTextEncoder", "patch_text_encoder", "unpatch_text_encoder",
    "get_keyframe_ind", "frame_errors", "select_keyframes", "resize_frames", "resize_image", "resize_size",
    "patch_keyframe_selection",
]
