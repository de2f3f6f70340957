"""ctypes binding of libmpx.so (include/mpx.h).  There is no CPU fallback: if the HIP library is
missing or a call fails, this module raises."""
import ctypes as C
import os

# torch first: PyTorch-ROCm ships its own libamdhip64; libmpx.so must bind to that one runtime (the
# one that owns the tensors and streams it is handed).  Loading libmpx.so before torch would pull
# /opt/rocm's copy into the process and the two runtimes do not share devices or streams.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPX_LIB_PATH: another build of the library for this process AND the processes it starts (tools/with_lib.py sets it for a probe
# build, so that `bench.py --gpus N`'s child ranks bind what the parent was told to bind); unset = the product library in the tree
PRODUCT_LIB_PATH = os.path.join(_HERE, "libmpx.so")
LIB_PATH = os.environ.get("MPX_LIB_PATH") or PRODUCT_LIB_PATH

IMG = 224
IMG_PAD = 230
NUM_CLASSES = 1000


class MpxError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("bn_name", C.c_char * 48),
                ("cin", C.c_int32), ("cout", C.c_int32), ("ksize", C.c_int32),
                ("stride", C.c_int32), ("pad", C.c_int32), ("hin", C.c_int32),
                ("hout", C.c_int32), ("relu", C.c_int32), ("residual", C.c_int32),
                ("k_packed", C.c_int32), ("cout_pad", C.c_int32)]


class NormDesc(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("channels", C.c_int32), ("hw", C.c_int32)]


class DwConvDesc(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("bn_name", C.c_char * 48), ("channels", C.c_int32), ("pitch", C.c_int32),
                ("stride", C.c_int32), ("hin", C.c_int32), ("clamp_in", C.c_int32)]


class SeDesc(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("channels", C.c_int32), ("pitch", C.c_int32), ("q", C.c_int32), ("hw", C.c_int32)]


class LnormDesc(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("channels", C.c_int32), ("hw", C.c_int32)]


class AttnDesc(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("tokens", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32)]


_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); must list every symbol include/mpx.h declares
SIGNATURES = {
    "mpx_create": (_i, [_i, _i, _i, C.POINTER(_vp)]),
    "mpx_destroy": (_i, [_vp]),
    "mpx_last_error": (C.c_char_p, [_vp]),
    "mpx_max_batch": (_i, [_vp]),
    "mpx_num_cus": (_i, [_vp]),
    "mpx_workspace_bytes": (C.c_size_t, [_vp]),
    "mpx_num_convs": (_i, [_vp]),
    "mpx_conv_info": (_i, [_vp, _i, C.POINTER(ConvDesc)]),
    "mpx_describe_plan": (_i, [_i, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "mpx_set_conv_weights": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f]),
    "mpx_geometry": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "mpx_mask_apply_minmax": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "mpx_avgpool2_pad": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mpx_weights_complete": (_i, [_vp]),
    "mpx_set_conv_tile": (_i, [_vp, _i, _i]),
    "mpx_get_conv_tile": (_i, [_vp, _i]),
    "mpx_last_conv_kernels": (_i, [_vp]),
    "mpx_pack_conv_weights": (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "mpx_mask_apply_normalize": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _fp, _fp, _i, _vp, _vp]),
    "mpx_stem_table_build": (_i, [_vp, _vp, _vp, _vp, _i, _fp, _fp, _vp]),
    "mpx_stem_table_apply": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "mpx_conv_bn_act": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mpx_conv_dual_bn_act": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mpx_set_fusion": (_i, [_vp, _i]),
    "mpx_bottleneck_tail": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mpx_num_bottleneck_tails": (_i, [_vp]),
    "mpx_bottleneck_tail_info": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "mpx_pointwise_tail": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mpx_num_pointwise_tails": (_i, [_vp]),
    "mpx_pointwise_tail_info": (_i, [_vp, _i, C.POINTER(_i), C.POINTER(_i)]),
    "mpx_stem_conv_maxpool": (_i, [_vp, _vp, _vp, _i, _vp]),
    "mpx_maxpool3x3s2": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_maxpool2x2s2": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_maxpool3x3s2p0": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_global_avgpool": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_head_softmax_gather": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mpx_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "mpx_heatmap_accumulate": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "mpx_input_planes": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mpx_mark_input_staged": (_i, [_vp, _i, _i]),
    "mpx_stem_planes": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mpx_profile_enable": (_i, [_vp, _i]),
    "mpx_profile_collect": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "mpx_flops_per_forward": (C.c_double, [_vp]),
    # DenseNet: the stand-alone BatchNorms, concat-append + BN + ReLU, the transitions' average pool
    "mpx_num_norms": (_i, [_vp]),
    "mpx_norm_info": (_i, [_vp, _i, C.POINTER(NormDesc)]),
    "mpx_load_norm": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _f]),
    "mpx_norm_params": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp)]),
    "mpx_concat_bn_relu": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, C.c_longlong, _vp]),
    "mpx_avgpool2x2s2": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_profile_collect_ex": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)]),
    # MobileNetV2: the depthwise layers, the depthwise 3x3 + BN + ReLU6 kernel, the clamped global pool
    "mpx_num_dwconvs": (_i, [_vp]),
    "mpx_dwconv_info": (_i, [_vp, _i, C.POINTER(DwConvDesc)]),
    "mpx_load_dwconv": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _f]),
    "mpx_dwconv_params": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mpx_dwconv3x3_bn_relu6": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mpx_global_avgpool_clamp6": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_profile_collect_dw": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # SqueezeNet 1.1: where a conv writes (the expand convs fill halves of one concatenation), the average pool that writes the logits
    "mpx_conv_out_slice": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_global_avgpool_logits": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    # GoogLeNet: the clipped-window 3x3 max pool, the pools of the forward, their launches in the profile
    "mpx_maxpool3x3_clip": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "mpx_num_clip_pools": (_i, [_vp]),
    "mpx_clip_pool_info": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_profile_collect_pool": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # ShuffleNetV2: the linear depthwise kernel, the channel shuffle, where a conv reads, the shuffles of the forward and their profile
    "mpx_dwconv3x3_bn": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mpx_dwconv_layout": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_shuffle2_concat": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mpx_num_shuffles": (_i, [_vp]),
    "mpx_shuffle_info": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_conv_in_slice": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_profile_collect_shuffle": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # EfficientNet-B0: the depthwise k x k + BN kernel with SiLU on either side, the SE layers, their gate and scale kernels, the SiLU pool
    "mpx_conv_consumer_act": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    "mpx_dwconv_shape": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_dwconv_bn_act": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "mpx_num_se": (_i, [_vp]),
    "mpx_se_info": (_i, [_vp, _i, C.POINTER(SeDesc)]),
    "mpx_load_se": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "mpx_se_params": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mpx_se_gate": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mpx_se_scale": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    # RegNetY: the SE gate with ReLU behind fc1, and which of the two gates an SE layer runs
    "mpx_se_gate_relu": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mpx_se_act": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    # RegNetX / RegNetY: the any-width grouped 3x3 kernel (tile 18) on the caller's planes, and its host packer
    "mpx_pack_gconvw_weights": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "mpx_gconvw3x3_bn_act": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "mpx_global_avgpool_silu": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_profile_collect_se": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong)] + [C.POINTER(C.c_double)] * 8),
    # ResNeXt: the groups of a layer (32 on a block's conv2, the grouped 3x3 kernel's layers)
    "mpx_conv_groups": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    # ConvNeXt: GELU in a conv's epilogue, the depthwise 7x7 + LayerNorm layers, the stand-alone LayerNorms, their three kernels
    "mpx_conv_epilogue_act": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    "mpx_dwconv_ln": (_i, [_vp, _i, C.POINTER(C.c_int), C.POINTER(_vp), C.POINTER(C.c_float)]),
    "mpx_load_dwconv_ln": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _f]),
    "mpx_num_lnorms": (_i, [_vp]),
    "mpx_lnorm_info": (_i, [_vp, _i, C.POINTER(LnormDesc)]),
    "mpx_load_lnorm": (_i, [_vp, _i, _vp, _vp, _f]),
    "mpx_lnorm_params": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_float)]),
    "mpx_dwconv7x7_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "mpx_layernorm_c": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, C.c_longlong, _i, _i, _vp]),
    "mpx_global_avgpool_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _i, _vp]),
    "mpx_profile_collect_ln": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong)] + [C.POINTER(C.c_double)] * 9),
    # ViT: the token layers' rows, the attention launches, class token + position embedding, the kernels of csrc/mpx_attn.h and the strided LayerNorm
    "mpx_conv_rows": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    "mpx_num_attn": (_i, [_vp]),
    "mpx_attn_info": (_i, [_vp, _i, C.POINTER(AttnDesc)]),
    "mpx_load_tokens": (_i, [_vp, _vp, _vp]),
    "mpx_token_params": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_attention": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mpx_tokens_assemble": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "mpx_layernorm_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, C.c_longlong, C.c_longlong, _i, _i, _vp]),
    "mpx_profile_collect_attn": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong)] + [C.POINTER(C.c_double)] * 11),
    # real-valued per-pixel masks (csrc/mpx_softmask.h): explicit weights or RISE's grids, applied like K0 and summed with the scores
    "mpx_softmask_apply": (_i, [_vp, _vp, _vp, _vp, _i, _fp, _fp, _i, _vp, _vp]),
    "mpx_rise_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _fp, _fp, _i, _vp, _vp]),
    "mpx_softmask_saliency": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "mpx_rise_saliency": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    # many classes from the same forwards (csrc/mpx_saliency_classes.h): K gathers per row of logits, the class-tiled saliency sums
    "mpx_softmax_gather_classes": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp]),
    "mpx_softmask_saliency_classes": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "mpx_rise_saliency_classes": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    # a second pixel source (csrc/mpx_rankmask.h): rows selected between the image and a fill image on a per-pixel rank; RISE's blur
    "mpx_rank_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _fp, _fp, _i, _vp, _vp]),
    "mpx_blur_fill": (_i, [_vp, _vp, _vp, _fp, _i, _fp, _fp, _vp, _vp]),
    # a linear surrogate over on/off rows (csrc/mpx_surrogate.h): the fp64 moment sums of LIME / KernelSHAP, the paint per superpixel
    "mpx_surrogate_accumulate": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mpx_segment_paint": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    # the rows of a Sobol total-order design over a d x d grid, gathered from the two design matrices in the apply kernel; the fill blend
    "mpx_sobol_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _fp, _fp, _i, _vp, _vp]),
    # occlusion sensitivity: one sliding box per row synthesised in the apply kernel; the overlap mean of the score drops (csrc/mpx_occlusion.h)
    "mpx_box_apply": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _fp, _fp, _i, _vp, _vp]),
    "mpx_box_saliency_classes": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
    "mpx_box_saliency_mean": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    # Score-CAM: the tap of the pool's input, the normalised cells, the maps upsampled in the apply kernel, the weighted sum (csrc/mpx_cam.h)
    "mpx_pool_input": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "mpx_planes_to_chw": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mpx_cam_cells": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "mpx_cam_apply": (_i, [_vp, _vp, _vp, _vp, _i, _i, _fp, _fp, _i, _vp, _vp]),
    "mpx_cam_combine": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
}

SOFTMASK_TILE = 32      # csrc/mpx_stage.h STAGE_MT: the rows one block of every apply kernel loops over ...
RANKMASK_TILE = SOFTMASK_TILE   # ... under the name the rank-mask tests know it by
SALIENCY_CLASS_TILE = 32    # csrc/mpx_saliency_classes.h SC_KT: the classes one thread of saliency_classes_kernel accumulates
SURROGATE_S_MAX = 1024     # csrc/mpx_surrogate.h SUR_S_MAX: the most superpixels mpx_surrogate_accumulate / mpx_segment_paint take
CAM_GRID_MIN, CAM_GRID_MAX = 2, 16     # include/mpx.h MPX_CAM_GRID_MIN / _MAX (csrc/mpx_softmask.h CAM_G_*): the map sides mpx_cam_apply / _cells / _combine take
SOBOL_GRID_MIN, SOBOL_GRID_MAX = 2, 32  # include/mpx.h MPX_SOBOL_GRID_MIN / _MAX (csrc/mpx_softmask.h SOBOL_GRID_*): the grids mpx_sobol_apply takes
OCCLUSION_BOX_TILE = 256    # csrc/mpx_occlusion.h OCC_BT: the boxes box_saliency_classes_kernel stages in LDS at a time
BLUR_KLEN_MAX = 31      # csrc/mpx_rankmask.h BF_KMAX: the most taps mpx_blur_fill takes

_lib = None


def load():
    """Load libmpx.so (built by __graft_entry__.build() / csrc/build.sh)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MpxError("HIP extension %s not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        if is_probe_build():
            import sys
            sys.stderr.write("mpx: binding %s (MPX_LIB_PATH / with_lib.py) -- NOT the product library %s; probe builds may be timing-only\n"
                             % (LIB_PATH, PRODUCT_LIB_PATH))
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)     # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def is_probe_build():
    """True when this process binds anything but the in-tree product library (MPX_LIB_PATH, tools/with_lib.py)."""
    return os.path.realpath(LIB_PATH) != os.path.realpath(PRODUCT_LIB_PATH)


def bound_library():
    """What a record of a run must carry to say WHICH library it ran (bench.py's config): the path this process binds, the
    sha256 of that file, the build stamp next to it (`<lib>.sha256` = __graft_entry__._source_hash of the sources and flags it was built
    from; None when there is none) and whether it is the in-tree product library."""
    import hashlib
    h = hashlib.sha256()
    with open(LIB_PATH, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 20), b""):
            h.update(chunk)
    stamp = None
    if os.path.exists(LIB_PATH + ".sha256"):
        with open(LIB_PATH + ".sha256") as fh:
            stamp = fh.read().strip()
    return {"lib_path": LIB_PATH, "lib_sha256": h.hexdigest(), "lib_stamp": stamp, "product_library": not is_probe_build()}


def check(handle, rc, what):
    if rc != 0:
        msg = load().mpx_last_error(handle).decode() if handle else ""
        raise MpxError("%s failed (rc=%d): %s" % (what, rc, msg))
