"""MI355X-native (gfx950) deformable convolution: the hot path of CHONSPQX/modulated-deform-conv
behind the reference's own operator surface.

    modulated_deform_conv_amd.MDCONV_CUDA              the 8 extension-module entry points
    modulated_deform_conv_amd.modulated_deform_conv    autograd Functions + nn.Modules
    modulated_deform_conv_amd.ops                      torch.library ops mdconv::deform_conv[_backward]
                                                       (fake kernels: torch.compile / export)
    modulated_deform_conv_amd.dcnv3                    the DCNv3 core operator (channels-last, fp32 / fp16 / bf16):
                                                       DCNv3Function, dcnv3_core, DCNv3, and DCNv3Fused (the same block
                                                       on the DCNv4 operator with its in-kernel softmax) -- also exported
                                                       here
    modulated_deform_conv_amd.msda                     multi-scale deformable attention (channels-last, fp32 / fp16 /
                                                       bf16, coordinates in the same type or fp32): MSDeformAttnFunction,
                                                       ms_deform_attn, ms_deform_attn_forward / _backward, MSDeformAttn
                                                       -- also exported here
    modulated_deform_conv_amd.dcnv4                    the DCNv4 operator (channels-last, one packed offset_mask tensor in
                                                       the values' dtype or fp32, remove_center, softmax): DCNv4Function,
                                                       dcnv4_core, dcnv4_forward / _backward, DCNv4 -- also exported here
    modulated_deform_conv_amd.fda                      packed deformable attention (one packed tensor of locations and
                                                       attention logits per (query, head), the softmax inside the
                                                       operator): FlashDeformAttnFunction, flash_deform_attn,
                                                       flash_deform_attn_forward / _backward, FlashDeformAttn,
                                                       pack_loc_attn / unpack_loc_attn -- also exported here
    modulated_deform_conv_amd.droi                     deformable RoI pooling (channels-last kernels behind logical NCHW
                                                       tensors, offsets in the same type or fp32): DeformRoIPoolFunction,
                                                       deform_roi_pool, deform_roi_pool_forward / _backward, DeformRoIPool,
                                                       DeformRoIPoolPack, ModulatedDeformRoIPoolPack -- also exported here
    modulated_deform_conv_amd.msda3d                   3-D multi-scale deformable attention over volumes (levels of
                                                       (T, H, W), locations (x, y, z), kernels of its own):
                                                       MSDeformAttn3DFunction, ms_deform_attn_3d,
                                                       ms_deform_attn_3d_forward / _backward, MSDeformAttn3D -- also
                                                       exported here
    modulated_deform_conv_amd.dagg                     deformable aggregation (Sparse4D / SparseDrive: key points sampled
                                                       from all cameras and levels in one call, C ABI in
                                                       include/mdconv_dagg.h): DeformableAggregationFunction,
                                                       deformable_aggregation, deformable_aggregation_forward / _backward,
                                                       feature_maps_format -- also exported here
    modulated_deform_conv_amd.msdap                    multi-scale deformable attention with a point count per level
                                                       (RT-DETRv2's num_points_list; D-FINE / DEIM: (3, 6, 3); C ABI in
                                                       include/mdconv_msdap.h): MSDeformAttnPointsFunction,
                                                       ms_deform_attn_points, ms_deform_attn_points_forward / _backward,
                                                       MSDeformableAttention -- also exported here
    modulated_deform_conv_amd.fdap                     packed deformable attention with a point count per level (one packed
                                                       tensor of locations and logits, the softmax over all K taps inside
                                                       the operator; C ABI in include/mdconv_fdap.h):
                                                       FlashDeformAttnPointsFunction, flash_deform_attn_points,
                                                       flash_deform_attn_points_forward / _backward,
                                                       MSDeformableAttentionFused, pack_loc_attn_points /
                                                       unpack_loc_attn_points -- also exported here
    modulated_deform_conv_amd.afda                     anchored packed deformable attention (the packed row of RAW offsets
                                                       and logits of one linear layer plus the reference points or boxes;
                                                       the reference arithmetic and the softmax inside the operator; C ABI
                                                       in include/mdconv_afda.h): AnchoredDeformAttnFunction,
                                                       anchored_deform_attn, anchored_deform_attn_forward / _backward,
                                                       MSDeformableAttentionAnchored -- also exported here
    modulated_deform_conv_amd.distributed              batch-sharded multi-GPU helper (RCCL)

All compute runs in libmdconv_hip.so (hand-written HIP, C ABI in include/mdconv.h); there is no
CPU or PyTorch fallback.
"""
from . import _capi  # noqa: F401  (does not load the library until first use)

__version__ = "0.1.0"

_DCNV3 = ("DCNv3Function", "dcnv3_core", "DCNv3", "DCNv3Fused")
_MSDA = ("ms_deform_attn_forward", "ms_deform_attn_backward", "MSDeformAttnFunction", "ms_deform_attn", "MSDeformAttn")
_DCNV4 = ("dcnv4_forward", "dcnv4_backward", "DCNv4Function", "dcnv4_core", "DCNv4")
_FDA = ("flash_deform_attn_forward", "flash_deform_attn_backward", "FlashDeformAttnFunction", "flash_deform_attn",
        "FlashDeformAttn", "pack_loc_attn", "unpack_loc_attn")
_DROI = ("deform_roi_pool_forward", "deform_roi_pool_backward", "DeformRoIPoolFunction", "deform_roi_pool", "DeformRoIPool",
         "DeformRoIPoolPack", "ModulatedDeformRoIPoolPack")
_MSDA3D = ("ms_deform_attn_3d_forward", "ms_deform_attn_3d_backward", "MSDeformAttn3DFunction", "ms_deform_attn_3d",
           "MSDeformAttn3D")
_DAGG = ("deformable_aggregation_forward", "deformable_aggregation_backward", "DeformableAggregationFunction",
         "deformable_aggregation", "feature_maps_format")
_MSDAP = ("ms_deform_attn_points_forward", "ms_deform_attn_points_backward", "MSDeformAttnPointsFunction",
          "ms_deform_attn_points", "MSDeformableAttention")
_FDAP = ("flash_deform_attn_points_forward", "flash_deform_attn_points_backward", "FlashDeformAttnPointsFunction",
         "flash_deform_attn_points", "MSDeformableAttentionFused", "pack_loc_attn_points", "unpack_loc_attn_points")
_AFDA = ("anchored_deform_attn_forward", "anchored_deform_attn_backward", "AnchoredDeformAttnFunction", "anchored_deform_attn",
         "MSDeformableAttentionAnchored")
__all__ = list(_DCNV3 + _MSDA + _DCNV4 + _FDA + _DROI + _MSDA3D + _DAGG + _MSDAP + _FDAP + _AFDA)


def __getattr__(name):
    # the DCNv3, MSDA, DCNv4 and packed-attention names resolve on first use, so importing the package stays as light as before
    if name in _DCNV3:
        from . import dcnv3
        return getattr(dcnv3, name)
    if name in _MSDA:
        from . import msda
        return getattr(msda, name)
    if name in _DCNV4:
        from . import dcnv4
        return getattr(dcnv4, name)
    if name in _FDA:
        from . import fda
        return getattr(fda, name)
    if name in _DROI:
        from . import droi
        return getattr(droi, name)
    if name in _MSDA3D:
        from . import msda3d
        return getattr(msda3d, name)
    if name in _DAGG:
        from . import dagg
        return getattr(dagg, name)
    if name in _MSDAP:
        from . import msdap
        return getattr(msdap, name)
    if name in _FDAP:
        from . import fdap
        return getattr(fdap, name)
    if name in _AFDA:
        from . import afda
        return getattr(afda, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
