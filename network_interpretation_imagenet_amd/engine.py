"""Host side of the masked-perturbation scorer: PyTorch-ROCm provides device memory and streams,
every computation is a hand-written HIP kernel behind the C-ABI of include/mpx.h.

Replaces the inner loop of the reference's three hot-path scripts
(generate_gp_training_data_imagenet.py:221-266, gp_superpixel_data_imagenet.py:276-334,
bayesian_active_learning_imagenet.py:170-218): mask build, `input * mask`, per-mask H2D copy,
batch-1 forward, per-mask D2H sync.  Here M masks of one image are staged and scored in one
batched launch sequence and only the M scores come back.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, masks
from ._lib import MpxError, IMG, NUM_CLASSES

# transforms.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
# generate_gp_training_data_imagenet.py:590-591
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-5   # torchvision BatchNorm2d default
GOOGLENET_BN_EPS = 1e-3     # torchvision googlenet.py: BasicConv2d = Conv2d(bias=False) + BatchNorm2d(eps=0.001) + ReLU

ARCH_IDS = {"resnet18": 18, "resnet34": 34, "resnet50": 50, "resnet101": 101, "resnet152": 152,
            # the reference's two small networks (include/mpx.h MPX_ARCH_*)
            "mnist_net": 1, "cifar_resnet20": 2020, "cifar_resnet56": 2056, "cifar_resnet110": 2110}
# torchvision's VGG networks (include/mpx.h MPX_ARCH_VGG / MPX_ARCH_VGG_BN + depth), which the reference's `-a` selects as well
ARCH_IDS.update({"vgg%d%s" % (d, bn): (3100 if bn else 3000) + d for d in (11, 13, 16, 19) for bn in ("", "_bn")})
ARCH_IDS["alexnet"] = 4000      # torchvision's AlexNet (MPX_ARCH_ALEXNET), the third family the reference's README names
# torchvision's DenseNets with growth rate 32 (MPX_ARCH_DENSENET + depth); densenet161 (growth rate 48) is not served
ARCH_IDS.update({"densenet%d" % d: 5000 + d for d in (121, 169, 201)})
ARCH_IDS["mobilenet_v2"] = 6002   # torchvision's MobileNetV2, width 1.0 (MPX_ARCH_MOBILENET + 2)
ARCH_IDS["squeezenet1_1"] = 7011  # torchvision's SqueezeNet 1.1 (MPX_ARCH_SQUEEZENET + 11); squeezenet1_0 is not served
ARCH_IDS["googlenet"] = 8000      # torchvision's GoogLeNet without the aux classifiers (MPX_ARCH_GOOGLENET); inception_v3 is not served
# torchvision's ShuffleNetV2 family (MPX_ARCH_SHUFFLENET + 10 x the width multiplier)
ARCH_IDS.update({"shufflenet_v2_x0_5": 9005, "shufflenet_v2_x1_0": 9010, "shufflenet_v2_x1_5": 9015, "shufflenet_v2_x2_0": 9020})
ARCH_IDS.update({"resnext50_32x4d": 11050, "resnext101_32x8d": 11101})    # torchvision's 32-group ResNeXts (MPX_ARCH_RESNEXT + 50 / 101); resnext101_64x4d and the Wide ResNets are not served
ARCH_IDS["efficientnet_b0"] = 10000     # torchvision's EfficientNet-B0 (MPX_ARCH_EFFICIENTNET + 0); B1 .. B7 (trained at 240 and more) are not served
ARCH_IDS.update({"convnext_tiny": 12001, "convnext_small": 12002})    # torchvision's ConvNeXts of width 96 (MPX_ARCH_CONVNEXT + 1 / 2); convnext_base / convnext_large are not served
CONVNEXT_LN_EPS = 1e-6      # torchvision convnext.py: every LayerNorm / LayerNorm2d is built with eps=1e-6
# torchvision's ViT-Base networks (MPX_ARCH_VIT + the patch size); vit_l_16 / vit_l_32 / vit_h_14 and the Swin family are not served.  The engine's
# descriptor names drop the leading "encoder.layers." (mpx_conv_desc.name holds 48 characters, "encoder.layers.encoder_layer_11.self_attention.
# out_proj" has 55): state_dict_name() puts it back, and in_proj's tensors are `...self_attention.in_proj_weight` / `in_proj_bias` (an
# underscore: nn.MultiheadAttention's own parameters, not a submodule's)
ARCH_IDS.update({"vit_b_16": 13016, "vit_b_32": 13032})
# torchvision's RegNetX networks up to 8 GF (MPX_ARCH_REGNET + ten times the GF figure): a bottleneck whose 3x3 is grouped by a fixed group width
ARCH_IDS.update({"regnet_x_400mf": 14004, "regnet_x_800mf": 14008, "regnet_x_1_6gf": 14016, "regnet_x_3_2gf": 14032, "regnet_x_8gf": 14080})
# torchvision's RegNetY networks from 800 MF to 8 GF (MPX_ARCH_REGNET_Y + ten times the GF figure): RegNetX's trunk with a Squeeze-and-Excitation
# gate (ReLU, sigmoid) in every block.  regnet_y_400mf (group width 8) and regnet_y_16gf / regnet_y_32gf (group widths 112 / 232) are not served
ARCH_IDS.update({"regnet_y_800mf": 15008, "regnet_y_1_6gf": 15016, "regnet_y_3_2gf": 15032, "regnet_y_8gf": 15080})
VIT_LN_EPS = 1e-6           # torchvision vision_transformer.py: norm_layer = partial(nn.LayerNorm, eps=1e-6)
VIT_LAYER_PREFIX = "encoder.layers."


def state_dict_name(name):
    """The state_dict prefix of a descriptor name: a ViT engine's "encoder_layer_<i>...." names get torchvision's "encoder.layers." back;
    every other name is its own prefix."""
    return VIT_LAYER_PREFIX + name if name.startswith("encoder_layer_") else name


COMPUTE_UNITS = 256        # MI355X; only what whole_round_batch falls back to when no GPU is visible (CPU tests, documentation)
ROUND_PIXELS_14 = 256      # pixels per tile of the kernels that run ONE workgroup per CU on the 14x14 maps (mpx_conv3p.h, mpx_conv256.h)


def device_compute_units(device=None):
    """Compute units of the GPU the engine will run on -- the number mpx_create reads (hipDeviceAttributeMultiprocessorCount; the
    engine reports it as MaskedForwardEngine.num_cus / mpx_num_cus) and the persistent kernels size their grids from.  256 on a
    whole MI355X; a partitioned or CU-masked device reports fewer.  Falls back to 256 without a GPU."""
    if torch.cuda.is_available():
        return int(torch.cuda.get_device_properties(torch.cuda.current_device() if device is None else device).multi_processor_count)
    return COMPUTE_UNITS


def whole_round_batch(limit, num_cus=None):
    """Largest forward batch <= `limit` whose 14x14 maps cut into whole rounds of 256-pixel tiles over the device's `num_cus`
    compute units (None = device_compute_units(); 256 CUs: 334.37 images per round).  The 3x3 patch kernel and the 256x256 tile
    keep one workgroup per CU, so a batch just ABOVE a whole number of rounds pays a whole extra round on the stage that holds
    2/3 of an ImageNet ResNet's time: measured on ResNet-101 (tools/batch_sweep.sh, profiles/r03_batch_sweep.txt) 44.8 us of
    conv time per masked image at 2006 / 2340 / 2674 / 3009 against 45.6-45.9 at 2010 and 2048.  Returns `limit` itself below
    one round."""
    per_round = (device_compute_units() if num_cus is None else int(num_cus)) * ROUND_PIXELS_14
    rounds = int(limit) * 196 // per_round
    if (rounds + 1) * per_round // 196 <= int(limit):       # the last tile of a batch may be partial: 2340 images are 1791.6 -> 1792 tiles
        rounds += 1
    return rounds * per_round // 196 if rounds >= 1 else int(limit)


def default_bn_eps(arch):
    """The epsilon of torchvision's BatchNorm layers in `arch`: BatchNorm2d's default 1e-5, except GoogLeNet's BasicConv2d (1e-3).  A
    ConvNeXt has no BatchNorm: the value is its LayerNorms' 1e-6."""
    if arch.startswith("convnext"):
        return CONVNEXT_LN_EPS
    if arch.startswith("vit_"):
        return VIT_LN_EPS
    return GOOGLENET_BN_EPS if arch == "googlenet" else BN_EPS


class BasePredictionWrong(Exception):
    """The unmasked prediction differs from the label; the reference only defines the scorer when
    it is correct (generate_gp_training_data_imagenet.py:215,269-273;
    bayesian_active_learning_imagenet.py:167,219-221)."""


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def rank_segments(segments):
    """Arbitrary integer label map -> (i32[224,224] ranks in np.unique(segments) order, S).
    The reference indexes superpixels through np.unique(segments)
    (generate_gp_training_data_imagenet.py:223,230)."""
    seg = np.asarray(segments)
    if seg.shape != (IMG, IMG):
        raise ValueError("segments must be [%d,%d], got %s" % (IMG, IMG, seg.shape))
    if not np.issubdtype(seg.dtype, np.integer):
        raise ValueError("segments must be an integer label map, got %s" % seg.dtype)
    # ranks in ascending label order = np.unique's order.  Label maps are small non-negative integers (felzenszwalb, grids, an already
    # ranked map): a histogram ranks them in one pass -- np.unique sorts 50,176 values (1 ms, twice per score_masks call, next to
    # ~7 ms of GPU time for a BO round's window table)
    flat = seg.reshape(-1)
    lo, hi = int(flat.min()), int(flat.max())
    if lo >= 0 and hi < 4 * flat.size:
        present = np.bincount(flat, minlength=hi + 1) > 0
        s = int(present.sum())
        if s == hi + 1:                                     # already 0 .. S-1 with no gap
            return np.ascontiguousarray(seg, dtype=np.int32), s
        rank = (np.cumsum(present) - 1).astype(np.int32)
        return rank[flat].reshape(IMG, IMG), s
    uniq, inv = np.unique(seg, return_inverse=True)
    return inv.reshape(IMG, IMG).astype(np.int32), int(len(uniq))


class _Packer:
    """The rows of consecutive jobs packed into forwards of up to max_batch slots (a job's rows may straddle two forwards); row g of the
    call reads label_rows[g] and writes score_out[g] / pred_out[g].  Allocates nothing, synchronises nothing."""

    def __init__(self, eng, label_rows, score_out, pred_out):
        self.eng, self.label_rows, self.score_out, self.pred_out = eng, label_rows, score_out, pred_out
        self.done, self.used, self.kind = 0, 0, None    # rows handed to a forward; slots staged for the next one; how those were staged

    def flush(self):
        at = slice(self.done, self.done + self.used)
        self.eng.forward(self.used, self.label_rows[at], score_out=self.score_out[at], pred_out=self.pred_out[at])
        self.done += self.used
        self.used = 0

    def add(self, rows, stage_fn):
        """stage_fn(r, take, slot0) stages rows [r, r + take) of a job into slots [slot0, slot0 + take); a full forward runs at once."""
        r = 0
        while r < rows:
            take = min(rows - r, self.eng.max_batch - self.used)
            stage_fn(r, take, self.used)
            self.used += take
            r += take
            if self.used == self.eng.max_batch:
                self.flush()

    def kind_changes(self, kind):       # a forward takes its slots from one kind of staging: a pending one of another kind runs now
        if self.used and kind != self.kind:
            self.flush()
        self.kind = kind

    def finish(self):
        if self.used:
            self.flush()


class MaskedForwardEngine:
    """One engine per process per GPU (one RCCL rank).  `arch` is the reference's `-a/--arch`."""

    def __init__(self, arch="resnet101", max_batch=None, device=None, stem=None, transform_input=False):
        """max_batch: slots of the workspace (masked images per forward); None = 512 for the ResNets and the small networks.  A VGG
        engine has no default: a VGG slot holds 26.5 MB (two 224x224x64 split-fp16 activation planes and the input staging, 1.8x a
        ResNet slot), so its caller sizes it -- MaskedForwardEngine("vgg16") raises ValueError, MaskedForwardEngine("vgg16",
        max_batch=512) is the size INTEGRATION.md 1 suggests.  An AlexNet slot holds 2.4 MB and keeps the default of 512.  A DenseNet slot
        holds 14.5 MB -- four 56x56x256 split-fp16 activation buffers (the block's raw concatenation, its normalised copy, conv1's and
        conv2's outputs: 12.8 MB), the input staging and the pooled stem planes, exactly a ResNet slot -- and keeps the default of 512.
        A MobileNetV2 slot holds 15.3 MB -- three 112x112x96 split-fp16 activation buffers (features.2's expanded map, 1.5x a ResNet
        buffer: 14.5 MB) and the input staging -- and keeps the default of 512 (7.8 GB).
        A SqueezeNet 1.1 slot holds 10.3 MB -- three 111x111x64 split-fp16 activation buffers (a Fire module's input, its squeeze map and
        the concatenation: 9.5 MB) and the input staging -- and keeps the default of 512 (5.3 GB).
        A GoogLeNet slot holds 10.5 MB -- three 112x112x64 split-fp16 activation buffers (the stem's output; a module's input, one branch's
        intermediate map and the concatenation: 9.6 MB) and the input staging -- and keeps the default of 512 (5.4 GB).
        A ShuffleNetV2 slot holds 5.7 MB for every width -- three 112x112x32 split-fp16 activation buffers (conv1's output, 24 channels at
        pitch 32; a block's input, its branch2 map and the shuffled output: 4.8 MB) and the input staging -- and keeps the default of 512
        (2.9 GB).
        An EfficientNet-B0 slot holds 15.3 MB -- three 112x112x96 split-fp16 activation buffers (features.2.0's expanded map, MobileNetV2's
        size: a block's input, its expanded map and the depthwise output the SE layer scales in place: 14.5 MB), the input staging and the
        SE gates -- and keeps the default of 512 (7.8 GB).
        A ResNeXt-50 32x4d slot is a ResNet slot (14.5 MB: its largest map is 56x56x256 too).  A ResNeXt-101 32x8d slot holds 27.3 MB -- four
        56x56x512 split-fp16 activation buffers (layer2.0.conv1's output: 25.7 MB), the input staging and the pooled stem planes -- and
        keeps the default of 512 (14 GB).
        A ConvNeXt-Tiny / -Small slot holds 15.3 MB -- three 56x56x384 split-fp16 activation buffers (block.3's output in stage 0,
        MobileNetV2's size: a block's input, its LayerNorm output and then its output, the hidden map: 14.5 MB) and the input staging -- and
        keeps the default of 512 (7.8 GB).
        A ViT-B/16 slot holds 6.3 MB -- four split-fp16 activation buffers of sizes of their own (the residual stream and a LayerNorm's /
        the attention's output, 197 x 768 each, in_proj's 197 x 2304 and the hidden 197 x 3072 rows: 5.45 MB) and the input staging --, a
        ViT-B/32 slot 2.2 MB (50 tokens); both keep the default of 512 (3.6 / 1.5 GB with the packed weights).
        A RegNetX slot holds four split-fp16 activation buffers of the network's largest map -- 112x112x32 (400MF: 7.3 MB with the input
        staging), 112x112x64 (800MF: 13.7 MB) or 112x112x96 (1.6GF, 3.2GF, 8GF: block1-0.f.a's output at a pitch of 96, 20.1 MB) -- and keeps
        the default of 512 (3.7 / 7.0 / 10.3 GB).  A RegNetY slot follows the same rule -- 112x112x64 (800MF), 112x112x64 (1.6GF: 48 channels at a
        pitch of 64), 112x112x96 (3.2GF) or 112x112x224 (8GF: 46 MB, 23.6 GB at 512) -- plus one gate row of the widest stage, and keeps 512 too.
        transform_input: torchvision's GoogLeNet flag (on in its pretrained model): a per-channel affine re-normalisation behind the
        caller's Normalize, after which a masked pixel is no longer 0.  The engine stages masked pixels as exact zeros and does not serve it:
        True raises ValueError; False, the default, is models.googlenet() without weights.
        stem: how score_packed / score_masks / score_images stage the masks of an image on the ImageNet ResNets --
        "table" (default): the stem by superposition (mpx_stem_table_build once per image, mpx_stem_table_apply per block of mask rows:
        K0, the stem conv and its max pool for all masks of an image without materialising a masked image) for every IMAGE that brings at
        least `stem_table_min_rows` (256) rows -- decided per image, however the rows are packed into calls and batches --, K0 + the MFMA
        stem otherwise (a BO round's 28 .. 118 windows); "conv": always
        K0 into the input staging, then the MFMA stem + max pool inside the forward (rounds 1-3).  stage_masks() is always K0."""
        if arch not in ARCH_IDS:
            raise ValueError("unsupported arch %r (torchvision ResNets, VGGs, AlexNet, DenseNets, MobileNetV2, SqueezeNet 1.1, GoogLeNet, ShuffleNetV2s and EfficientNet-B0 and the reference's small networks, and torchvision's ResNeXt-50 32x4d / ResNeXt-101 32x8d, ConvNeXt-Tiny / -Small, ViT-B/16 / ViT-B/32, RegNetX-400MF .. -8GF and RegNetY-800MF .. -8GF: %s)" % (arch, sorted(ARCH_IDS)))
        if transform_input:
            raise ValueError("%s: transform_input=True is not served -- the engine stages masked pixels as exact zeros, and torchvision's "
                             "re-normalisation behind the caller's Normalize would move them (INTEGRATION.md)" % arch)
        if max_batch is None:
            if arch.startswith("vgg"):
                raise ValueError("%s: pass max_batch -- a VGG engine holds 26.5 MB per slot and has no default size "
                                 "(max_batch=512: 14 GB, INTEGRATION.md 1)" % arch)
            max_batch = 512
        if not torch.cuda.is_available():
            raise MpxError("no MI355X visible: the scorer has no CPU path")
        self._lib = _lib.load()
        self.arch = arch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.max_batch = int(max_batch)
        h = C.c_void_p()
        rc = self._lib.mpx_create(ARCH_IDS[arch], self.max_batch, self.device.index, C.byref(h))
        if rc != 0:
            raise MpxError("mpx_create(%s, max_batch=%d) failed rc=%d" % (arch, max_batch, rc))
        self._h = h
        self.layers = []
        for i in range(self._lib.mpx_num_convs(h)):
            d = _lib.ConvDesc()
            _lib.check(h, self._lib.mpx_conv_info(h, i, C.byref(d)), "mpx_conv_info")
            self.layers.append(d)
        self.norms = []         # the BatchNorms that precede their conv (DenseNet: every norm1, the transitions' norm, norm5)
        for k in range(self._lib.mpx_num_norms(h)):
            nd = _lib.NormDesc()
            _lib.check(h, self._lib.mpx_norm_info(h, k, C.byref(nd)), "mpx_norm_info")
            self.norms.append(nd)
        self.dwconvs = []       # the depthwise 3x3 layers (MobileNetV2), a list of their own next to the conv list
        for k in range(self._lib.mpx_num_dwconvs(h)):
            dd = _lib.DwConvDesc()
            _lib.check(h, self._lib.mpx_dwconv_info(h, k, C.byref(dd)), "mpx_dwconv_info")
            self.dwconvs.append(dd)
        self.dw_ksizes = []     # their kernel sizes (3; 5 on EfficientNet-B0's stages 3, 5 and 6): what mpx_dwconv_desc has no field for
        for k in range(len(self.dwconvs)):
            ks = C.c_int()
            _lib.check(h, self._lib.mpx_dwconv_shape(h, k, C.byref(ks), None, None), "mpx_dwconv_shape")
            self.dw_ksizes.append(int(ks.value))
        self.dw_ln = []         # 1 where the layer is a ConvNeXt block's depthwise 7x7 with bias and the LayerNorm fused behind it (mpx_dwconv_ln)
        for k in range(len(self.dwconvs)):
            ln = C.c_int()
            _lib.check(h, self._lib.mpx_dwconv_ln(h, k, C.byref(ln), None, None), "mpx_dwconv_ln")
            self.dw_ln.append(int(ln.value))
        self.lnorms = []        # the LayerNorms that are launches of their own (ConvNeXt: the stem's, the downsample norms, classifier.0)
        for k in range(self._lib.mpx_num_lnorms(h)):
            ld = _lib.LnormDesc()
            _lib.check(h, self._lib.mpx_lnorm_info(h, k, C.byref(ld)), "mpx_lnorm_info")
            self.lnorms.append(ld)
        self.epilogue_acts = []     # per conv layer: 1 = exact GELU in its epilogue (a ConvNeXt block.3), 0 everywhere else
        for i in range(len(self.layers)):
            a = C.c_int()
            _lib.check(h, self._lib.mpx_conv_epilogue_act(h, i, C.byref(a)), "mpx_conv_epilogue_act")
            self.epilogue_acts.append(int(a.value))
        self.conv_rows = []     # per conv layer: the rows per image of a ViT's token layers (197 / 50; their descriptors say hin = hout = 0), 0 everywhere else
        for i in range(len(self.layers)):
            r = C.c_int()
            _lib.check(h, self._lib.mpx_conv_rows(h, i, C.byref(r)), "mpx_conv_rows")
            self.conv_rows.append(int(r.value))
        self.attns = []         # the attention launches (ViT: one per encoder layer), a list of their own
        for k in range(self._lib.mpx_num_attn(h)):
            ad = _lib.AttnDesc()
            _lib.check(h, self._lib.mpx_attn_info(h, k, C.byref(ad)), "mpx_attn_info")
            self.attns.append(ad)
        self.ses = []           # the Squeeze-and-Excitation layers (EfficientNet-B0, RegNetY), a list of their own as well
        for k in range(self._lib.mpx_num_se(h)):
            sd_ = _lib.SeDesc()
            _lib.check(h, self._lib.mpx_se_info(h, k, C.byref(sd_)), "mpx_se_info")
            self.ses.append(sd_)
        self.se_acts = []       # per SE layer: fc1's activation, 0 SiLU (EfficientNet-B0), 1 ReLU (RegNetY)
        for k in range(len(self.ses)):
            a = C.c_int()
            _lib.check(h, self._lib.mpx_se_act(h, k, C.byref(a)), "mpx_se_act")
            self.se_acts.append(int(a.value))
        self.groups = []        # groups per conv layer: 32 on a ResNeXt block's conv2 (weight [cout][cin / 32][3][3]), width / group width on a RegNetX / RegNetY block's f.b, 1 everywhere else
        for i in range(len(self.layers)):
            gr = C.c_int()
            _lib.check(h, self._lib.mpx_conv_groups(h, i, C.byref(gr)), "mpx_conv_groups")
            self.groups.append(int(gr.value))
        self.flops_per_forward = float(self._lib.mpx_flops_per_forward(h))
        self.num_cus = int(self._lib.mpx_num_cus(h))        # what the persistent kernels' grids are sized from (whole_round_batch)
        self._mean, self._std = _f3(MEAN), _f3(STD)
        g = [C.c_int() for _ in range(4)]
        _lib.check(h, self._lib.mpx_geometry(h, *[C.byref(v) for v in g]), "mpx_geometry")
        self.image_size, self.in_channels, self.num_classes, self.logit_pitch = (int(v.value) for v in g)
        self.small = self.image_size != IMG
        # below this many mask rows per image the table does not pay for every label map: building it costs what K0 + the MFMA stem cost
        # for ~40 masks and a short apply launch leaves the chip half empty.  tools/stem_bench.py, ms per 2340 rows, table / K0 + MFMA
        # stem: 16-pixel grid 96 rows per image 3.2 / 3.6, 256 rows 1.9 / 3.5, 512 rows 1.5 / 3.5; the (fragmented) felzenszwalb fixture
        # 96 rows 5.5 / 3.7, 256 rows 3.1 / 3.5, 512 rows 2.3 / 3.6 -- at 256 no map loses
        self.stem_table_min_rows = 256
        if stem not in (None, "table", "conv"):
            raise ValueError("stem must be 'table' or 'conv', got %r" % (stem,))
        if not self.has_stem_table and stem == "table":
            raise ValueError("%s has no 7x7 stem: stem='table' is the ImageNet ResNets' path" % arch)
        self.stem = (stem or "table") if self.has_stem_table else "conv"
        self._last_batch = 0    # the slots the last forward ran (pool_input taps no other)

    @property
    def has_stem_table(self):
        """The stem by superposition needs the ImageNet ResNets' 7x7 stem + max pool; VGG, AlexNet, DenseNet (whose stem has that shape, but
        which keeps no table), MobileNetV2, SqueezeNet 1.1, GoogLeNet (that stem shape again, but another pool behind it), the ShuffleNetV2s,
        EfficientNet-B0, the ConvNeXts (a 4x4 stride-4 patchify stem, no pool), the ViTs (a 16x16 / 32x32 patchify stem), the RegNetXs and RegNetYs (a 3x3
        stride-2 stem, no pool) and the small networks stage through K0 only."""
        return not self.small and not getattr(self, "arch", "").startswith(("vgg", "alexnet", "densenet", "mobilenet", "squeezenet", "googlenet", "shufflenet", "efficientnet", "convnext", "vit_", "regnet"))

    def stem_for_rows(self, rows_per_image):
        """The staging an IMAGE that brings `rows_per_image` mask rows to a job gets on this engine: "table" (the stem by superposition) from
        `stem_table_min_rows` rows on, "conv" (K0 + the MFMA stem) below or when the engine was created with stem="conv".  The two stagings
        round differently (<= 2.5e-6 on a score), so whoever SPLITS a job -- shard.score_masks_sharded / heatmap_sharded over ranks, a caller
        cutting an image's rows into several calls -- decides ONCE from the job's row count with this function and hands the answer to
        every call as `stem=`: the shards then carry the bits of the unsplit call."""
        return "table" if (self.stem == "table" and int(rows_per_image) >= self.stem_table_min_rows) else "conv"

    def _staging(self, stem, rows):
        """Resolve the `stem=` argument for ONE image that brings `rows` mask rows: None = stem_for_rows(rows), else the caller's choice."""
        if stem is None:
            return self.stem_for_rows(rows)
        if stem not in ("table", "conv"):
            raise ValueError("stem must be None, 'table' or 'conv', got %r" % (stem,))
        if stem == "table" and not self.has_stem_table:
            raise ValueError("%s has no 7x7 stem: stem='table' is the ImageNet ResNets' path" % self.arch)
        return stem

    # ---- life cycle ----
    def close(self):
        if getattr(self, "_h", None):
            self._lib.mpx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def eval(self):
        """nn.Module.eval() of the reference (generate_gp_training_data_imagenet.py:159): the engine
        only has the inference mode (BatchNorm running statistics)."""
        return self

    def cuda(self):
        return self

    @property
    def workspace_bytes(self):
        return int(self._lib.mpx_workspace_bytes(self._h))

    # ---- weights ----
    def load_state_dict(self, sd, eps=None, only=None):
        """`sd`: torchvision ResNet / ResNeXt (conv2.weight [width][width / 32][3][3], what mpx_conv_groups says) / VGG / AlexNet / DenseNet / MobileNetV2 / SqueezeNet 1.1 / GoogLeNet / ShuffleNetV2 / EfficientNet-B0 state_dict (key names as `models.<arch>().state_dict()`), e.g.
        torch.load(local_path, weights_only=True); keys the engine has no use for (`num_batches_tracked`, the `aux1.` / `aux2.` classifiers
        of torchvision's GoogLeNet checkpoint) are ignored.  `eps`: the BatchNorms' epsilon; None = default_bn_eps(arch), torchvision's value
        for the architecture (1e-5; 1e-3 for googlenet).  `module.` prefixes (DataParallel) are accepted.  `only`: conv names
        ("layer1.1.conv3", "fc") to (re)load instead of every layer -- the engine rebuilds whatever it derived from a reloaded
        layer (the K-concatenated conv3 | downsample planes, a block tail's permuted copy).  MobileNetV2's and ShuffleNetV2's depthwise layers
        load with the convs, and `only` takes their names ("features.2.conv.1.0", "stage2.0.branch1.0") too.  A ShuffleNetV2 state_dict loads
        as saved: the engine places the columns of a layer that reads a two-half stage map itself.  EfficientNet-B0's depthwise and
        Squeeze-and-Excitation layers load with the convs too (fc1 / fc2 weight and bias of every `features.S.B.block.J`), and `only` takes
        the SE layers' names as well; so do a RegNetY's (`trunk_output.blockS.blockS-J.f.se`)."""
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        if eps is None:
            eps = default_bn_eps(self.arch)
        if only is not None:
            only = set(only)
            unknown = only - {d.name.decode() for d in self.layers} - {d.name.decode() for d in self.dwconvs} - {d.name.decode() for d in self.ses}
            if unknown:
                raise KeyError("no such conv layers: %s" % sorted(unknown))

        def get(key, shape):
            if key not in sd:
                raise KeyError("state_dict lacks %r" % key)
            t = sd[key].detach().to("cpu", torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError("%s has shape %s, expected %s" % (key, tuple(t.shape), shape))
            return t

        for i, d in enumerate(self.layers):
            name, bn = d.name.decode(), d.bn_name.decode()
            if only is not None and name not in only:
                continue
            w4 = (d.cout, d.cin // self.groups[i], d.ksize, d.ksize)
            if self.attns:
                # a ViT: every layer is bias-only -- the ordinary epilogue with gamma 1, beta 0, mean 0, var 1, eps 0 (scale = 2^-e, shift =
                # bias exactly, as ConvNeXt's block.5 carries its layer scale); in_proj's tensors have an underscore in their names
                full = state_dict_name(name)
                wkey, bkey = (full + "_weight", full + "_bias") if name.endswith(".in_proj") else (full + ".weight", full + ".bias")
                w = get(wkey, w4 if d.ksize > 1 else (d.cout, d.cin)).reshape(w4).contiguous()
                cb = get(bkey, (d.cout,))
                zero, one = torch.zeros(d.cout), torch.ones(d.cout)
                _lib.check(self._h, self._lib.mpx_set_conv_weights(self._h, i, _ptr(w), _ptr(cb), _ptr(one), _ptr(zero), _ptr(zero), _ptr(one), 0.0),
                           "mpx_set_conv_weights(%s)" % name)
                continue
            wshape = (d.cout, w4[1] * d.ksize * d.ksize) if (name + ".weight") in sd and sd[name + ".weight"].dim() == 2 else w4
            # a Linear layer as a conv: VGG's classifier.0 is [4096, 25088] = [4096, 512 * 7 * 7] (AlexNet's classifier.1 [4096, 256 * 6 * 6]), channel-major as torch.flatten of NCHW
            w = get(name + ".weight", wshape).reshape(w4).contiguous()
            layer_eps = eps
            if bn.endswith(".layer_scale"):
                # ConvNeXt's block.5: fc2 + layer scale + residual is the ordinary epilogue with the layer scale as gamma over mean 0,
                # var 1, eps 0 and beta 0 -- scale = layer_scale * 2^-e, shift = bias * layer_scale, exactly
                cb = get(name + ".bias", (d.cout,))
                g = get(bn, (d.cout, 1, 1)).reshape(d.cout).contiguous()
                zero, one = torch.zeros(d.cout), torch.ones(d.cout)
                args = (_ptr(w), _ptr(cb), _ptr(g), _ptr(zero), _ptr(zero), _ptr(one))
                layer_eps = 0.0
            elif not bn and self.norms and i != len(self.layers) - 1:
                # DenseNet's conv2 / transition convs: no BatchNorm behind them, no ReLU and no bias (scale = 2^-e, shift = 0)
                args = (_ptr(w), None, None, None, None, None)
            elif not bn:        # no BatchNorm: fc, or the MNIST net's conv6 -- the layer's own bias goes in as `beta`
                b = get(name + ".bias", (d.cout,))
                args = (_ptr(w), None, None, _ptr(b), None, None)
            else:
                cb = get(name + ".bias", (d.cout,)) if (name + ".bias") in sd else None      # nn.Conv2d(bias=True) + BN
                g = get(bn + ".weight", (d.cout,))
                b = get(bn + ".bias", (d.cout,))
                m = get(bn + ".running_mean", (d.cout,))
                v = get(bn + ".running_var", (d.cout,))
                args = (_ptr(w), _ptr(cb), _ptr(g), _ptr(b), _ptr(m), _ptr(v))
            _lib.check(self._h, self._lib.mpx_set_conv_weights(self._h, i, *args, float(layer_eps)),
                       "mpx_set_conv_weights(%s)" % name)
        for k, dd in enumerate(self.dwconvs):
            name, bn = dd.name.decode(), dd.bn_name.decode()
            if only is not None and name not in only:
                continue
            if self.dw_ln[k]:       # ConvNeXt: depthwise 7x7 with bias, `bn` is the LayerNorm behind it
                t = [get(name + ".weight", (dd.channels, 1, self.dw_ksizes[k], self.dw_ksizes[k])), get(name + ".bias", (dd.channels,)),
                     get(bn + ".weight", (dd.channels,)), get(bn + ".bias", (dd.channels,))]
                _lib.check(self._h, self._lib.mpx_load_dwconv_ln(self._h, k, *[_ptr(v) for v in t], float(eps)), "mpx_load_dwconv_ln(%s)" % name)
                continue
            t = [get(name + ".weight", (dd.channels, 1, self.dw_ksizes[k], self.dw_ksizes[k]))]
            t += [get("%s.%s" % (bn, key), (dd.channels,)) for key in ("weight", "bias", "running_mean", "running_var")]
            _lib.check(self._h, self._lib.mpx_load_dwconv(self._h, k, *[_ptr(v) for v in t], float(eps)), "mpx_load_dwconv(%s)" % name)
        for k, se in enumerate(self.ses):
            name = se.name.decode()
            if only is not None and name not in only:
                continue
            t = [get(name + ".fc1.weight", (se.q, se.channels, 1, 1)), get(name + ".fc1.bias", (se.q,)),
                 get(name + ".fc2.weight", (se.channels, se.q, 1, 1)), get(name + ".fc2.bias", (se.channels,))]
            _lib.check(self._h, self._lib.mpx_load_se(self._h, k, *[_ptr(v) for v in t]), "mpx_load_se(%s)" % name)
        if only is None:        # the stand-alone BatchNorms belong to no conv: a full load brings them all
            for k, nd in enumerate(self.norms):
                name = nd.name.decode()
                t = [get("%s.%s" % (name, key), (nd.channels,)) for key in ("weight", "bias", "running_mean", "running_var")]
                _lib.check(self._h, self._lib.mpx_load_norm(self._h, k, *[_ptr(v) for v in t], float(eps)), "mpx_load_norm(%s)" % name)
            for k, ld in enumerate(self.lnorms):        # ... and so do ConvNeXt's stand-alone LayerNorms
                name = state_dict_name(ld.name.decode())
                t = [get(name + ".weight", (ld.channels,)), get(name + ".bias", (ld.channels,))]
                _lib.check(self._h, self._lib.mpx_load_lnorm(self._h, k, *[_ptr(v) for v in t], float(eps)), "mpx_load_lnorm(%s)" % name)
            if self.attns:      # ... and a ViT's class token and position embedding
                tk, wd = C.c_int(), C.c_int()
                _lib.check(self._h, self._lib.mpx_token_params(self._h, None, None, C.byref(tk), C.byref(wd)), "mpx_token_params")
                t = [get("class_token", (1, 1, wd.value)), get("encoder.pos_embedding", (1, tk.value, wd.value))]
                _lib.check(self._h, self._lib.mpx_load_tokens(self._h, *[_ptr(v) for v in t]), "mpx_load_tokens")
        return self

    # ---- kernels ----
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _image_ptrs(self, image):
        """(u8 pointer, f32 pointer) of a device image, one of them None: raw u8[224,224,3] or normalised f32[3,224,224]."""
        if image.dtype == torch.uint8 and tuple(image.shape) == (IMG, IMG, 3):
            return _ptr(image), None
        if image.dtype == torch.float32 and tuple(image.shape) == (3, IMG, IMG):
            return None, _ptr(image)
        raise ValueError("image must be uint8[224,224,3] or float32[3,224,224], got %s%s" % (image.dtype, tuple(image.shape)))

    def _require_imagenet(self):
        if self.small:
            raise ValueError("%s scores with score_masks_removed (the small networks' mask convention)" % self.arch)

    def stage_masks(self, image, seg, onoff, slot0=0, out_f32=None):
        """K0.  image: device u8[224,224,3] (raw) or f32[3,224,224] (normalised); seg: device
        i32[224,224] ranks; onoff: device u8[M,S].  Fills input slots [slot0, slot0+M)."""
        for name, t in (("image", image), ("seg", seg), ("onoff", onoff)):
            if t.device != self.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous tensor on %s" % (name, self.device))
        if seg.dtype != torch.int32 or tuple(seg.shape) != (IMG, IMG):
            raise ValueError("seg must be int32[%d,%d]" % (IMG, IMG))
        if onoff.dtype != torch.uint8 or onoff.dim() != 2:
            raise ValueError("onoff must be uint8[M,S]")
        m, s = onoff.shape
        u8, f32 = self._image_ptrs(image)
        if out_f32 is not None and (out_f32.dtype != torch.float32 or tuple(out_f32.shape) != (m, 3, IMG, IMG)
                                    or not out_f32.is_contiguous()):
            raise ValueError("out_f32 must be contiguous float32[M,3,224,224]")
        _lib.check(self._h, self._lib.mpx_mask_apply_normalize(
            self._h, u8, f32, _ptr(seg), _ptr(onoff), int(m), int(s), self._mean, self._std,
            int(slot0), _ptr(out_f32), self._stream()), "mpx_mask_apply_normalize")

    def build_stem_table(self, image, seg, num_segments):
        """mpx_stem_table_build: the mask-independent terms of the stem for ONE image (device u8[224,224,3] or f32[3,224,224]) and its
        rank map (device i32[224,224], labels in [0, num_segments)); the engine holds one table at a time."""
        for name, t in (("image", image), ("seg", seg)):
            if t.device != self.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous tensor on %s" % (name, self.device))
        if seg.dtype != torch.int32 or tuple(seg.shape) != (IMG, IMG):
            raise ValueError("seg must be int32[%d,%d]" % (IMG, IMG))
        u8, f32 = self._image_ptrs(image)
        _lib.check(self._h, self._lib.mpx_stem_table_build(self._h, u8, f32, _ptr(seg), int(num_segments), self._mean, self._std,
                                                           self._stream()), "mpx_stem_table_build")

    def apply_stem_table(self, onoff, slot0=0):
        """mpx_stem_table_apply: the pooled stem output of M mask rows (device u8[M,S]) of the image whose table is in place, into slots
        [slot0, slot0+M); the next forward over those slots starts behind the max pool."""
        if onoff.device != self.device or not onoff.is_contiguous() or onoff.dtype != torch.uint8 or onoff.dim() != 2:
            raise ValueError("onoff must be a contiguous uint8[M,S] tensor on %s" % self.device)
        m, s = onoff.shape
        _lib.check(self._h, self._lib.mpx_stem_table_apply(self._h, _ptr(onoff), int(m), int(s), int(slot0), self._stream()),
                   "mpx_stem_table_apply")

    def forward(self, batch, labels, want_logits=False, score_out=None, pred_out=None):
        """Whole network over the staged slots [0,batch).  labels: device i32[batch].
        returns (score f32[batch], pred i32[batch][, logits f32[batch,1000]]) on the device; score_out / pred_out
        (contiguous device tensors of that shape and dtype) receive the results without any allocation."""
        if labels.dtype != torch.int32 or labels.device != self.device or labels.numel() != batch or not labels.is_contiguous():
            raise ValueError("labels must be contiguous int32[%d] on %s" % (batch, self.device))
        for name, t, dt in (("score_out", score_out, torch.float32), ("pred_out", pred_out, torch.int32)):
            if t is not None and (t.dtype != dt or t.device != self.device or t.numel() != batch or not t.is_contiguous()):
                raise ValueError("%s must be contiguous %s[%d] on %s" % (name, dt, batch, self.device))
        score = score_out if score_out is not None else torch.empty(batch, dtype=torch.float32, device=self.device)
        pred = pred_out if pred_out is not None else torch.empty(batch, dtype=torch.int32, device=self.device)
        logits = torch.empty(batch, self.logit_pitch, dtype=torch.float32, device=self.device) if want_logits else None
        _lib.check(self._h, self._lib.mpx_forward(self._h, _ptr(labels), _ptr(score), _ptr(pred), _ptr(logits),
                                                  int(batch), self._stream()), "mpx_forward")
        self._last_batch = int(batch)
        return (score, pred, logits[:, :self.num_classes]) if want_logits else (score, pred)

    def input_plane_shape(self, n):
        """Shape of n slots of the engine's input staging: [n,230,230,4] (padded NHWC4, the 7x7 stem's operand) for the ImageNet
        ResNets, [n,H,W,32] (channels padded to 32) for the small networks (csrc/mpx_api.hip mpx_create)."""
        if self.small:
            return (int(n), self.image_size, self.image_size, 32)
        return (int(n), _lib.IMG_PAD, _lib.IMG_PAD, 4)

    def input_planes(self, n=None):
        """Zero-copy fp16 views of the engine-owned input staging planes (hi, lo), shaped input_plane_shape(n).
        For tests and diagnostics; reading them changes nothing.  Whoever WRITES slots by hand calls mark_input_staged() before forward()."""
        n = self.max_batch if n is None else int(n)
        if not 0 < n <= self.max_batch:
            raise ValueError("input_planes: n must be in [1, max_batch=%d]" % self.max_batch)
        hi, lo = C.c_void_p(), C.c_void_p()
        _lib.check(self._h, self._lib.mpx_input_planes(self._h, C.byref(hi), C.byref(lo)), "mpx_input_planes")
        return self._plane_views(hi.value, lo.value, self.input_plane_shape(n))

    def _plane_views(self, ptr_hi, ptr_lo, shape):
        """Zero-copy fp16 tensors of that shape over two engine-owned device planes."""
        class _View:
            def __init__(self, ptr):
                self.__cuda_array_interface__ = {"data": (ptr, False), "shape": shape, "typestr": "<f2", "version": 2}

        return torch.as_tensor(_View(ptr_hi), device=self.device), torch.as_tensor(_View(ptr_lo), device=self.device)

    def mark_input_staged(self, slot0, m):
        """mpx_mark_input_staged: slots [slot0, slot0+m) of the input planes were written by hand -- the next forward runs the stem on them."""
        _lib.check(self._h, self._lib.mpx_mark_input_staged(self._h, int(slot0), int(m)), "mpx_mark_input_staged")

    def stem_planes(self, n=None):
        """Zero-copy fp16 views (hi, lo) [n,56,56,64] of the engine-owned pooled stem output planes (ImageNet ResNets).  For tests."""
        n = self.max_batch if n is None else int(n)
        if not self.has_stem_table or not 0 < n <= self.max_batch:
            raise ValueError("stem_planes: an ImageNet ResNet engine and n in [1, max_batch=%d]" % self.max_batch)
        hi, lo = C.c_void_p(), C.c_void_p()
        _lib.check(self._h, self._lib.mpx_stem_planes(self._h, C.byref(hi), C.byref(lo)), "mpx_stem_planes")
        return self._plane_views(hi.value, lo.value, (n, 56, 56, 64))

    # ---- the batched surface ----
    def _image_to_device(self, image):
        t = torch.as_tensor(image)
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dtype == torch.uint8:
            if tuple(t.shape) != (IMG, IMG, 3):
                raise ValueError("uint8 image must be [224,224,3] (HWC), got %s" % (tuple(t.shape),))
        elif t.dtype == torch.float32:
            if tuple(t.shape) != (3, IMG, IMG):
                raise ValueError("float32 image must be [3,224,224] (normalised CHW), got %s" % (tuple(t.shape),))
        else:
            raise ValueError("image must be uint8 HWC or float32 CHW, got %s" % t.dtype)
        return t.contiguous().to(self.device)

    @staticmethod
    def _host_onoff(onoff, s, name="onoff"):
        """Host on/off rows as a contiguous uint8[M, S] array; S = the number of labels of the job's label map."""
        onoff = np.ascontiguousarray(onoff)
        if onoff.dtype != np.uint8 or onoff.ndim != 2 or onoff.shape[1] != s:
            raise ValueError("%s must be uint8[M,%d] (S = number of distinct segment labels), got %s%s" % (name, s, onoff.dtype, onoff.shape))
        return onoff

    def score_masks_removed(self, image_chw, segments, removed, label, return_logits=False, return_inputs=False):
        """The small networks' scorer: (image f32[C,H,W] as the loader yields it, segments int[H,W],
        removed u8[M,S] with 1 = superpixel switched OFF, label) -> (removed, score f32[M], pred i32[M][, logits][, inputs]).
        The mask convention is generate_gp_training_data_cifar.py:274-321 / generate_gp_training_data_mnist.py:167-242:
        min-max the picture to [0,255], multiply by the {0,255} mask, min-max again, * f32(1/255); pred[m] is the reference's
        `pred_mask`, score[m] the softmax probability of `label`."""
        if not self.small:
            raise ValueError("score_masks_removed is the small networks' convention; %s uses score_masks" % self.arch)
        x = torch.as_tensor(image_chw)
        if x.dim() == 4 and x.shape[0] == 1:
            x = x[0]
        n = self.image_size
        if x.dtype != torch.float32 or tuple(x.shape) != (self.in_channels, n, n):
            raise ValueError("image must be float32[%d,%d,%d], got %s%s" % (self.in_channels, n, n, x.dtype, tuple(x.shape)))
        seg = np.asarray(segments)
        if seg.shape != (n, n) or not np.issubdtype(seg.dtype, np.integer):
            raise ValueError("segments must be an integer [%d,%d] label map" % (n, n))
        uniq, inv = np.unique(seg, return_inverse=True)
        s = int(len(uniq))
        removed = np.ascontiguousarray(removed)
        if removed.dtype != np.uint8 or removed.ndim != 2 or removed.shape[1] != s:
            raise ValueError("removed must be uint8[M,%d], got %s%s" % (s, removed.dtype, removed.shape))
        if not 0 <= int(label) < self.num_classes:
            raise ValueError("label %r outside [0,%d)" % (label, self.num_classes))
        m = removed.shape[0]
        score = np.empty(m, dtype=np.float32)
        pred = np.empty(m, dtype=np.int32)
        logits = np.empty((m, self.num_classes), dtype=np.float32) if return_logits else None
        inputs = np.empty((m, self.in_channels, n, n), dtype=np.float32) if return_inputs else None
        x_d = x.contiguous().to(self.device)
        seg_d = torch.from_numpy(inv.reshape(n, n).astype(np.int32)).to(self.device)
        rem_d = torch.from_numpy(removed).to(self.device)
        for s0 in range(0, m, self.max_batch):
            b = min(self.max_batch, m - s0)
            labels = torch.full((b,), int(label), dtype=torch.int32, device=self.device)
            out_f32 = torch.empty(b, self.in_channels, n, n, dtype=torch.float32, device=self.device) if return_inputs else None
            _lib.check(self._h, self._lib.mpx_mask_apply_minmax(self._h, _ptr(x_d), _ptr(seg_d), _ptr(rem_d[s0:s0 + b].contiguous()),
                                                                int(b), int(s), 0, _ptr(out_f32), self._stream()),
                       "mpx_mask_apply_minmax")
            out = self.forward(b, labels, want_logits=return_logits)
            score[s0:s0 + b] = out[0].cpu().numpy()
            pred[s0:s0 + b] = out[1].cpu().numpy()
            if return_logits:
                logits[s0:s0 + b] = out[2].cpu().numpy()
            if return_inputs:
                inputs[s0:s0 + b] = out_f32.cpu().numpy()
        res = (removed, score, pred)
        if return_logits:
            res += (logits,)
        if return_inputs:
            res += (inputs,)
        return res

    def score_masks(self, image, segments, onoff, label, return_logits=False, stem=None):
        """(image, segments, onoff u8[M,S], label) -> (onoff u8[M,S], score f32[M], pred i32[M]).
        score[m] = softmax(model(normalised_image * mask_m))[label]
        (bayesian_active_learning_imagenet.py:187-198); pred[m] == label is the generators' binary
        label (generate_gp_training_data_imagenet.py:248,257).  stem: None = staged by this call's row count (stem_for_rows(M)); "table" /
        "conv" = the caller's choice -- a caller that scores PART of an image's rows passes stem_for_rows(all of them)."""
        self._require_imagenet()
        seg_rank, s = rank_segments(segments)
        onoff = self._host_onoff(onoff, s)
        if not 0 <= int(label) < NUM_CLASSES:
            raise ValueError("label %r outside [0,1000)" % (label,))
        m = onoff.shape[0]
        if not return_logits:
            # one upload, forwards of max_batch slots back to back, ONE download at the end (no per-chunk synchronisation)
            score, pred = self.score_images([image], [seg_rank], [onoff], [label], stem=stem)[0]
            return onoff, score, pred
        if m == 0:          # nothing is uploaded and `stem` is not looked at
            return onoff, np.empty(0, dtype=np.float32), np.empty(0, dtype=np.int32), np.empty((0, NUM_CLASSES), dtype=np.float32)
        stage = self._onoff_job(image, seg_rank, onoff, stem)[0]
        return (onoff,) + self._score_staged(m, stage, label, True)

    def score_packed(self, images, segs, onoffs, label_rows, score_out, pred_out, stem=None):
        """Device-resident packed scoring: the mask rows of SEVERAL images share forward batches of up to max_batch slots
        (an image's rows may straddle two batches), so the network always runs at the batch size it is fast at -- the
        reference scores one mask per forward (generate_gp_training_data_imagenet.py:240-248,
        gp_superpixel_data_imagenet.py:299-307).  images: sequence of device tensors (u8[224,224,3] or f32[3,224,224]);
        segs: ONE device i32[224,224] rank map shared by all images, or a sequence with one per image; onoffs: sequence of
        device u8[M_i, S_i]; label_rows: device i32[sum M_i] (image i's label repeated M_i times); score_out f32 / pred_out
        i32 [sum M_i] receive the results.  Allocates nothing, synchronises nothing.  Staging is decided PER IMAGE, from that image's own
        row count: `stem` = None stages image i by stem_for_rows(M_i) (the table from stem_table_min_rows rows on, K0 + the MFMA stem below),
        "table" / "conv" force one kind for every image of the call (a caller that hands over PART of an image's rows passes
        stem_for_rows(all of them)).  A forward takes its slots from one kind of staging (mpx_forward refuses a mixed batch), so the pending
        forward is flushed where the kind changes between consecutive images -- callers that can reorder (score_images) group the images by
        kind first.  A row's bits depend neither on where it sits in a batch nor on what else the call scores (kernel choice does not depend
        on the position of a mask, staging only on the row's own image): results are bit-identical to scoring every image on its own."""
        n = len(images)
        shared = isinstance(segs, torch.Tensor)
        if len(onoffs) != n or (not shared and len(segs) != n):
            raise ValueError("images, segs and onoffs must have one entry per image")
        total = sum(int(o.shape[0]) for o in onoffs)
        for name, t, dt in (("label_rows", label_rows, torch.int32), ("score_out", score_out, torch.float32), ("pred_out", pred_out, torch.int32)):
            if t.dtype != dt or t.device != self.device or t.numel() != total or not t.is_contiguous():
                raise ValueError("%s must be contiguous %s[%d] on %s" % (name, dt, total, self.device))
        label_rows, score_out, pred_out = label_rows.view(-1), score_out.view(-1), pred_out.view(-1)
        if stem is not None:
            self._staging(stem, 0)
        pack = _Packer(self, label_rows, score_out, pred_out)
        for i in range(n):
            m, image, onoff = int(onoffs[i].shape[0]), images[i], onoffs[i]
            if not m:
                continue
            seg = segs if shared else segs[i]
            kind = self.stem_for_rows(m) if stem is None else stem
            pack.kind_changes(kind)     # one forward, one kind of staging
            if kind == "table":
                self.build_stem_table(image, seg, int(onoff.shape[1]))      # once per image; its rows follow in one or two forwards
                pack.add(m, lambda r, take, slot0: self.apply_stem_table(onoff[r:r + take], slot0))
            else:
                pack.add(m, lambda r, take, slot0: self.stage_masks(image, seg, onoff[r:r + take], slot0))
        pack.finish()

    def score_images(self, images, segments, onoffs, labels, stem=None):
        """Host convenience over score_packed: [(image, segments, onoff u8[M_i,S_i], label)] for several images ->
        [(score f32[M_i], pred i32[M_i])], with ONE upload of the inputs and ONE download of all scores.  `segments` are
        arbitrary integer label maps (ranked here as score_masks does); `stem` as in score_packed: None stages every image by its own row
        count, so an image gets the same bits here as when it is scored alone, whatever it is packed with."""
        self._require_imagenet()
        n = len(images)
        if not (len(segments) == len(onoffs) == len(labels) == n):
            raise ValueError("images, segments, onoffs and labels must have the same length")
        self._staging(stem, 0)           # a bad `stem` fails here, whatever the rows
        img_d, seg_d, onoff_d, lab, sizes = [], [], [], [], []
        for i in range(n):
            seg_rank, s = rank_segments(segments[i])
            o = self._host_onoff(onoffs[i], s, "onoffs[%d]" % i)
            if not 0 <= int(labels[i]) < NUM_CLASSES:
                raise ValueError("label %r outside [0,1000)" % (labels[i],))
            sizes.append(o.shape[0])
            if o.shape[0] == 0:
                continue
            img_d.append(self._image_to_device(images[i]))
            seg_d.append(torch.from_numpy(seg_rank).to(self.device))
            onoff_d.append(torch.from_numpy(o).to(self.device))
            lab.append(np.full(o.shape[0], int(labels[i]), dtype=np.int32))
        total = int(sum(sizes))
        if total == 0:
            return [(np.empty(0, np.float32), np.empty(0, np.int32)) for _ in range(n)]
        # every image is staged by ITS OWN row count (score_packed); the images of one kind go first so that the forward is flushed at most
        # once for the change of kind (stable: the order within a kind is the caller's)
        order = list(range(len(img_d)))
        if stem is None:
            order.sort(key=lambda k: self.stem_for_rows(int(onoff_d[k].shape[0])) != "table")
        label_rows = torch.from_numpy(np.concatenate([lab[k] for k in order])).to(self.device)
        score = torch.empty(total, dtype=torch.float32, device=self.device)
        pred = torch.empty(total, dtype=torch.int32, device=self.device)
        self.score_packed([img_d[k] for k in order], [seg_d[k] for k in order], [onoff_d[k] for k in order], label_rows, score, pred, stem=stem)
        score, pred = score.cpu().numpy(), pred.cpu().numpy()
        packed, at = {}, 0
        for k in order:
            m = int(onoff_d[k].shape[0])
            packed[k] = (score[at:at + m].copy(), pred[at:at + m].copy())
            at += m
        out, k = [], 0
        for m in sizes:
            if m == 0:
                out.append((np.empty(0, np.float32), np.empty(0, np.int32)))
            else:
                out.append(packed[k])
                k += 1
        return out

    def predict(self, image):
        """Unmasked forward: (argmax class, softmax f32[1000])
        (generate_gp_training_data_imagenet.py:193,202)."""
        seg = np.zeros((IMG, IMG), dtype=np.int32)
        _o, _s, pred, logits = self.score_masks(image, seg, np.ones((1, 1), dtype=np.uint8), 0, return_logits=True)
        z = logits[0].astype(np.float64)
        p = np.exp(z - z.max())
        return int(pred[0]), (p / p.sum()).astype(np.float32)

    def heatmap_accumulate(self, seg, onoff, pred, labels, heat):
        """K5: heat[p] += sum_m [pred[m] == labels[m]] * onoff[m][seg[p]] on the device
        (gp_superpixel_data_imagenet.py:322-323).  seg i32[224,224], onoff u8[M,S], pred/labels i32[M],
        heat f32[224,224] -- all device tensors; heat is updated in place."""
        m, s = onoff.shape
        for name, t, dt in (("seg", seg, torch.int32), ("onoff", onoff, torch.uint8), ("pred", pred, torch.int32),
                            ("labels", labels, torch.int32), ("heat", heat, torch.float32)):
            if t.device != self.device or t.dtype != dt or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s tensor on %s" % (name, dt, self.device))
        if tuple(seg.shape) != (IMG, IMG) or tuple(heat.shape) != (IMG, IMG) or pred.numel() != m or labels.numel() != m:
            raise ValueError("shapes: seg/heat [224,224], pred/labels [M], onoff [M,S]")
        _lib.check(self._h, self._lib.mpx_heatmap_accumulate(self._h, _ptr(seg), _ptr(onoff), _ptr(pred), _ptr(labels),
                                                             int(m), int(s), _ptr(heat), self._stream()),
                   "mpx_heatmap_accumulate")
        return heat

    def heatmap_device(self, image, seg_rank, onoff, label, buf, stem=None):
        """Score the M mask-vectors of one image and accumulate their heat map WITHOUT a host round trip:
        buf (device f32[224*224 + 1]) gets heat[p] += sum_m [pred[m] == label] * onoff[m][seg[p]] in its first 224*224 elements
        (K5, gp_superpixel_data_imagenet.py:322-323) and the number of correctly predicted masks added to its last element --
        the layout shard.heatmap_sharded closes with ONE all_reduce (which passes stem_for_rows(the image's rows over ALL ranks) as `stem`).
        -> (score f32[M], pred i32[M]) device tensors."""
        if buf.dtype != torch.float32 or buf.device != self.device or buf.numel() != IMG * IMG + 1 or not buf.is_contiguous():
            raise ValueError("buf must be a contiguous float32[%d] tensor on %s" % (IMG * IMG + 1, self.device))
        seg_rank, s = rank_segments(seg_rank)               # a rank map passes through on the histogram's fast path
        onoff = self._host_onoff(onoff, s)
        if not 0 <= int(label) < NUM_CLASSES:
            raise ValueError("label %r outside [0,1000)" % (label,))
        m = int(onoff.shape[0])
        self._staging(stem, m)
        score = torch.empty(m, dtype=torch.float32, device=self.device)
        pred = torch.empty(m, dtype=torch.int32, device=self.device)
        if m == 0:
            return score, pred
        seg_d = torch.from_numpy(seg_rank).to(self.device)
        onoff_d = torch.from_numpy(onoff).to(self.device)
        labels = torch.full((m,), int(label), dtype=torch.int32, device=self.device)
        self.score_packed([self._image_to_device(image)], seg_d, [onoff_d], labels, score, pred, stem=stem)
        self.heatmap_accumulate(seg_d, onoff_d, pred, labels, buf[:IMG * IMG].view(IMG, IMG))
        buf[IMG * IMG] += (pred == labels).sum()
        return score, pred

    def heatmap(self, seg_rank, onoff, pred, label):
        """Host-array convenience over K5: -> f64[224,224] = sum_m [pred[m] == label] * onoff[m][seg[p]]
        (counts are integers < 2^24, so the f32 accumulation on the device is exact)."""
        m = int(np.asarray(onoff).shape[0])
        heat = torch.zeros(IMG, IMG, dtype=torch.float32, device=self.device)
        if m:
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
            self.heatmap_accumulate(t(seg_rank, np.int32), t(onoff, np.uint8), t(pred, np.int32),
                                    torch.full((m,), int(label), dtype=torch.int32, device=self.device), heat)
        return heat.cpu().numpy().astype(np.float64)

    # ---- real-valued per-pixel masks (csrc/mpx_softmask.h): explicit weights, RISE's grids ----
    def _soft_args(self, image, out_f32, m):
        """(u8 pointer, f32 pointer) of a device image for the soft-mask apply entries, with stage_masks' checks."""
        if image.device != self.device or not image.is_contiguous():
            raise ValueError("image must be a contiguous tensor on %s" % self.device)
        ptrs = self._image_ptrs(image)
        if out_f32 is not None and (out_f32.dtype != torch.float32 or tuple(out_f32.shape) != (m, 3, IMG, IMG)
                                    or out_f32.device != self.device or not out_f32.is_contiguous()):
            raise ValueError("out_f32 must be contiguous float32[M,3,224,224] on %s" % self.device)
        return ptrs

    def _soft_weights(self, weights):
        if (weights.device != self.device or weights.dtype != torch.float32 or weights.dim() != 3 or tuple(weights.shape[1:]) != (IMG, IMG)
                or not weights.is_contiguous()):
            raise ValueError("weights must be a contiguous float32[M,224,224] tensor on %s" % self.device)
        return int(weights.shape[0])

    def _rise_grids(self, cells, shifts, s):
        s = int(s)
        if not masks.RISE_S_MIN <= s <= masks.RISE_S_MAX:
            raise ValueError("s=%r outside [%d, %d]" % (s, masks.RISE_S_MIN, masks.RISE_S_MAX))
        if (cells.device != self.device or cells.dtype != torch.uint8 or cells.dim() != 3 or tuple(cells.shape[1:]) != (s, s)
                or not cells.is_contiguous()):
            raise ValueError("cells must be a contiguous uint8[M,%d,%d] tensor on %s" % (s, s, self.device))
        m = int(cells.shape[0])
        if shifts.device != self.device or shifts.dtype != torch.int32 or tuple(shifts.shape) != (m, 2) or not shifts.is_contiguous():
            raise ValueError("shifts must be a contiguous int32[%d,2] tensor on %s" % (m, self.device))
        return m, s

    def stage_soft_masks(self, image, weights, slot0=0, out_f32=None):
        """mpx_softmask_apply: K0 with a weight per pixel.  image as stage_masks; weights: device f32[M,224,224].  Fills input slots
        [slot0, slot0+M) with normalised image * weights[m] (one fp32 multiply, then the hi / lo split); binary weights give K0's planes bit for bit."""
        m = self._soft_weights(weights)
        u8, f32 = self._soft_args(image, out_f32, m)
        _lib.check(self._h, self._lib.mpx_softmask_apply(self._h, u8, f32, _ptr(weights), m, self._mean, self._std, int(slot0),
                                                         _ptr(out_f32), self._stream()), "mpx_softmask_apply")

    def stage_rise(self, image, cells, shifts, s, slot0=0, out_f32=None):
        """mpx_rise_apply: the same with RISE's weights synthesised in the kernel from cells (device u8[M,s,s], non-zero = keep) and shifts
        (device i32[M,2] = (dy, dx)); the weights are masks.rise_weights(cells, shifts, s) bit for bit.  The shifts are the caller's contract
        (each in [0, ceil(224 / s)); masks.check_rise verifies host arrays before they are uploaded)."""
        m, s = self._rise_grids(cells, shifts, s)
        u8, f32 = self._soft_args(image, out_f32, m)
        _lib.check(self._h, self._lib.mpx_rise_apply(self._h, u8, f32, _ptr(cells), _ptr(shifts), m, s, self._mean, self._std, int(slot0),
                                                     _ptr(out_f32), self._stream()), "mpx_rise_apply")

    def _sal_args(self, weight, sal, m):
        if weight.device != self.device or weight.dtype != torch.float32 or weight.numel() != m or not weight.is_contiguous():
            raise ValueError("weight must be a contiguous float32[%d] tensor on %s" % (m, self.device))
        self._sal_map(sal)

    def _sal_map(self, sal):
        if sal.device != self.device or sal.dtype != torch.float32 or tuple(sal.shape) != (IMG, IMG) or not sal.is_contiguous():
            raise ValueError("sal must be a contiguous float32[224,224] tensor on %s" % self.device)

    def _sal_out(self, out, k=None):
        """The zeroed device map(s) a saliency driver sums into: the caller's `out` (checked, f32[224,224] or f32[k,224,224]) or new ones."""
        shape = (IMG, IMG) if k is None else (k, IMG, IMG)
        sal = torch.zeros(shape, dtype=torch.float32, device=self.device) if out is None else out
        self._sal_map(sal) if k is None else self._sal_maps(sal, k)
        return sal.zero_() if out is not None else sal

    @staticmethod
    def _sal_return(sal, out):
        """A host array, or the caller's device tensor in its place (nothing is downloaded)."""
        return sal.cpu().numpy() if out is None else sal

    def soft_saliency_accumulate(self, weights, weight, sal):
        """mpx_softmask_saliency: sal[p] <- sal[p] + weight[m] * weights[m][p] for m ascending, in place, on the device (a rounded multiply and
        a rounded add per step; one thread per pixel, so the bits do not depend on how the rows are cut into calls).  weights: device
        f32[M,224,224]; weight: device f32[M], e.g. the scores of the forward that just ran; sal: device f32[224,224]."""
        m = self._soft_weights(weights)
        self._sal_args(weight, sal, m)
        _lib.check(self._h, self._lib.mpx_softmask_saliency(self._h, _ptr(weights), _ptr(weight), m, _ptr(sal), self._stream()),
                   "mpx_softmask_saliency")
        return sal

    def rise_saliency_accumulate(self, cells, shifts, s, weight, sal):
        """mpx_rise_saliency: soft_saliency_accumulate with the weights synthesised from RISE's cells and shifts (as stage_rise)."""
        m, s = self._rise_grids(cells, shifts, s)
        self._sal_args(weight, sal, m)
        _lib.check(self._h, self._lib.mpx_rise_saliency(self._h, _ptr(cells), _ptr(shifts), _ptr(weight), m, s, _ptr(sal), self._stream()),
                   "mpx_rise_saliency")
        return sal

    def _score_staged(self, m, stage, label, return_logits, after=None):
        """Forwards of up to max_batch slots over m rows that stage(s0, b) writes into slots [0, b), always through the input staging (the
        conv path: a real-valued mask has no stem table).  Scores and predictions stay on the device until ONE download at the end;
        after(s0, b, score_chunk), if given, runs behind each forward.  -> (score f32[m], pred i32[m][, logits f32[m,1000]]) host arrays."""
        self._require_imagenet()
        if not 0 <= int(label) < NUM_CLASSES:
            raise ValueError("label %r outside [0,1000)" % (label,))
        score = torch.empty(m, dtype=torch.float32, device=self.device)
        pred = torch.empty(m, dtype=torch.int32, device=self.device)
        labels = torch.full((min(m, self.max_batch),), int(label), dtype=torch.int32, device=self.device)
        rows = []
        for s0 in range(0, m, self.max_batch):
            b = min(self.max_batch, m - s0)
            stage(s0, b)
            out = self.forward(b, labels[:b], want_logits=return_logits, score_out=score[s0:s0 + b], pred_out=pred[s0:s0 + b])
            if return_logits:
                rows.append(out[2].cpu().numpy())
            if after is not None:
                after(s0, b, score[s0:s0 + b])
        res = (score.cpu().numpy(), pred.cpu().numpy())
        if return_logits:
            res += (np.concatenate(rows) if rows else np.empty((0, NUM_CLASSES), dtype=np.float32),)
        return res

    def score_soft_masks(self, image, weights, label, return_logits=False):
        """(image, weights f32[M,224,224], label) -> (score f32[M], pred i32[M][, logits f32[M,1000]]):
        score[m] = softmax(model(normalised_image * weights[m]))[label] for real-valued per-pixel masks (soft-edged occlusion windows, RISE
        masks built elsewhere, ...).  The masked images are never materialised: each chunk of max_batch weight maps is uploaded and staged
        by mpx_softmask_apply.  Always the conv staging; for weights in {0, 1} the scores are score_masks(..., stem="conv")'s bit for bit."""
        w = np.ascontiguousarray(weights)
        if w.dtype != np.float32 or w.ndim != 3 or w.shape[1:] != (IMG, IMG):
            raise ValueError("weights must be float32[M,224,224], got %s%s" % (w.dtype, w.shape))
        img_d = self._image_to_device(image)

        def stage(s0, b):
            self.stage_soft_masks(img_d, torch.from_numpy(w[s0:s0 + b]).to(self.device), 0)

        return self._score_staged(int(w.shape[0]), stage, label, return_logits)

    def score_rise(self, image, cells, shifts, s, label, return_logits=False):
        """(image, cells u8[M,s,s], shifts i32[M,2], s, label) -> (score f32[M], pred i32[M][, logits f32[M,1000]]): the scores of RISE's
        masks (masks.rise_cells / masks.rise_shifts), whose weights masks.rise_weights(cells, shifts, s) are synthesised in the apply
        kernel -- s * s bytes and a shift go to the device per mask instead of a 200 KB weight map.  Shifts outside [0, ceil(224 / s)) and
        s outside [2, 32] are refused here, before anything is uploaded."""
        cells, shifts = masks.check_rise(cells, shifts, s)
        img_d = self._image_to_device(image)
        cells_d, shifts_d = torch.from_numpy(cells).to(self.device), torch.from_numpy(shifts).to(self.device)

        def stage(s0, b):
            self.stage_rise(img_d, cells_d[s0:s0 + b], shifts_d[s0:s0 + b], s, 0)

        return self._score_staged(int(cells.shape[0]), stage, label, return_logits)

    def rise_saliency(self, image, label, n_masks=4000, s=7, p1=0.5, seed=0, out=None):
        """RISE's saliency map of `label` (Petsiuk, Das, Saenko, BMVC 2018): sum_m score[m] * w_m / (n_masks * p1) over n_masks random masks --
        cells, shifts = masks.rise_masks(n_masks, s, p1, seed).  Chunks of max_batch masks run apply -> forward -> accumulation on the device
        (mpx_rise_apply, mpx_forward, mpx_rise_saliency) with no host round trip in between; the sum is fp32 in mask order.
        out: None -> a host f32[224,224]; a contiguous device f32[224,224] is overwritten with the map and returned (nothing is downloaded)."""
        if not 0.0 < float(p1) <= 1.0 or int(n_masks) <= 0:
            raise ValueError("n_masks > 0 and p1 in (0, 1], got n_masks=%r p1=%r" % (n_masks, p1))
        cells, shifts = masks.rise_masks(n_masks, s, p1, seed)
        sal = self._sal_out(out)
        img_d = self._image_to_device(image)
        cells_d, shifts_d = torch.from_numpy(cells).to(self.device), torch.from_numpy(shifts).to(self.device)

        def stage(s0, b):
            self.stage_rise(img_d, cells_d[s0:s0 + b], shifts_d[s0:s0 + b], s, 0)

        def after(s0, b, score):
            self.rise_saliency_accumulate(cells_d[s0:s0 + b], shifts_d[s0:s0 + b], s, score, sal)

        self._score_staged(int(n_masks), stage, label, False, after=after)
        return self._sal_return(sal.div_(float(n_masks) * float(p1)), out)

    # ---- many classes from the same forwards (csrc/mpx_saliency_classes.h): K gathers per row of logits, the class-tiled sums ----
    def _classes_to_device(self, classes):
        """None (all classes) or a device i32[K] tensor of a host sequence / tensor of class indices -> (device tensor or None, K)."""
        if classes is None:
            return None, self.num_classes
        t = classes if isinstance(classes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(classes, dtype=np.int32))
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() == 0:
            raise ValueError("classes must be a non-empty int32[K], got %s%s" % (t.dtype, tuple(t.shape)))
        return t.contiguous().to(self.device), int(t.numel())

    def _class_score_rows(self, scores, m, k, name="scores"):
        """Rows of class scores: device f32[m, k] whose rows lie score_pitch = stride(0) >= k floats apart -> score_pitch."""
        if (scores.device != self.device or scores.dtype != torch.float32 or tuple(scores.shape) != (m, k) or scores.stride(1) != 1
                or (m > 1 and scores.stride(0) < k)):
            raise ValueError("%s must be a float32[%d,%d] tensor on %s with unit column stride and a row stride >= %d"
                             % (name, m, k, self.device, k))
        return int(scores.stride(0)) if m > 1 else max(int(scores.stride(0)), k)

    def class_scores(self, logits, classes=None, out=None):
        """mpx_softmax_gather_classes: device f32[B, K], out[b][k] = softmax(logits[b])[classes[k]] -- the head's score for label classes[k]
        bit for bit, for K classes of the same rows.  logits: what forward(want_logits=True) returns (device f32[B, num_classes], rows
        logit_pitch apart); classes: None (all num_classes classes, K = num_classes) or int32[K] (a class outside [0, num_classes) scores
        0.0); out: a device f32[B, K] with unit column stride (a column block of a wider tensor: its padding is not written)."""
        if (logits.device != self.device or logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[0] == 0
                or logits.shape[1] not in (self.num_classes, self.logit_pitch) or logits.stride(1) != 1
                or (logits.shape[0] > 1 and logits.stride(0) != self.logit_pitch)):
            raise ValueError("logits must be float32[B,%d] on %s with rows %d floats apart (forward(want_logits=True))"
                             % (self.num_classes, self.device, self.logit_pitch))
        b = int(logits.shape[0])
        cls_d, k = self._classes_to_device(classes)
        if out is None:
            out = torch.empty(b, k, dtype=torch.float32, device=self.device)
        pitch = self._class_score_rows(out, b, k, "out")
        _lib.check(self._h, self._lib.mpx_softmax_gather_classes(self._h, _ptr(logits), _ptr(cls_d), k, _ptr(out), pitch, b, self._stream()),
                   "mpx_softmax_gather_classes")
        return out

    def _sal_maps(self, sal, k):
        if sal.device != self.device or sal.dtype != torch.float32 or tuple(sal.shape) != (k, IMG, IMG) or not sal.is_contiguous():
            raise ValueError("sal must be a contiguous float32[%d,224,224] tensor on %s" % (k, self.device))

    def _sal_classes_args(self, scores, sal, m):
        if scores.dim() != 2 or sal.dim() != 3:
            raise ValueError("scores must be float32[M,K] and sal float32[K,224,224]")
        k = int(sal.shape[0])
        self._sal_maps(sal, k)
        return k, self._class_score_rows(scores, m, k)

    def soft_saliency_accumulate_classes(self, weights, scores, sal):
        """mpx_softmask_saliency_classes: sal[k][p] <- sal[k][p] + scores[m][k] * weights[m][p] for m ascending, in place (a rounded multiply
        and a rounded add per step).  Map k is soft_saliency_accumulate(weights, scores[:, k], sal[k]) bit for bit; every weight is read once
        per tile of _lib.SALIENCY_CLASS_TILE classes.  weights: device f32[M,224,224]; scores: device f32[M,K] (class_scores' output);
        sal: device f32[K,224,224]."""
        m = self._soft_weights(weights)
        k, pitch = self._sal_classes_args(scores, sal, m)
        _lib.check(self._h, self._lib.mpx_softmask_saliency_classes(self._h, _ptr(weights), _ptr(scores), pitch, m, k, _ptr(sal),
                                                                    self._stream()), "mpx_softmask_saliency_classes")
        return sal

    def rise_saliency_accumulate_classes(self, cells, shifts, s, scores, sal):
        """mpx_rise_saliency_classes: soft_saliency_accumulate_classes with the weights synthesised from RISE's cells and shifts (as
        stage_rise), once per mask and pixel for a whole tile of classes."""
        m, s = self._rise_grids(cells, shifts, s)
        k, pitch = self._sal_classes_args(scores, sal, m)
        _lib.check(self._h, self._lib.mpx_rise_saliency_classes(self._h, _ptr(cells), _ptr(shifts), _ptr(scores), pitch, m, k, s, _ptr(sal),
                                                                self._stream()), "mpx_rise_saliency_classes")
        return sal

    def _score_classes_staged(self, m, stage, cls_d, k, after=None):
        """_score_staged's loop with the logits kept: chunks of up to max_batch rows run stage(s0, b) -> forward(want_logits=True) ->
        class_scores on the stream; after(s0, b, scores_chunk), if given, runs behind each chunk.  -> (scores f32[m, k], pred i32[m]) on
        the device.  The two loops differ in the step behind stage(): the head's gather of one label there, class_scores of the kept logits
        here; score_masks_removed's loop differs in kind (another apply entry, a download of out_f32 per chunk)."""
        self._require_imagenet()
        scores = torch.empty(m, k, dtype=torch.float32, device=self.device)
        pred = torch.empty(m, dtype=torch.int32, device=self.device)
        labels = torch.zeros(min(m, self.max_batch), dtype=torch.int32, device=self.device)    # the head's own gather is not used
        unused = torch.empty_like(labels, dtype=torch.float32)
        for s0 in range(0, m, self.max_batch):
            b = min(self.max_batch, m - s0)
            stage(s0, b)
            logits = self.forward(b, labels[:b], want_logits=True, score_out=unused[:b], pred_out=pred[s0:s0 + b])[2]
            self.class_scores(logits, cls_d, out=scores[s0:s0 + b])
            if after is not None:
                after(s0, b, scores[s0:s0 + b])
        return scores, pred

    def score_soft_masks_classes(self, image, weights, classes):
        """score_soft_masks for several classes of the same forwards: -> (scores f32[M,K], pred i32[M]); column i is
        score_soft_masks(image, weights, classes[i])'s scores bit for bit.  classes: a sequence of class indices, or None for all."""
        cls = masks.class_selection(classes, None, NUM_CLASSES)[0]
        w = np.ascontiguousarray(weights)
        if w.dtype != np.float32 or w.ndim != 3 or w.shape[1:] != (IMG, IMG):
            raise ValueError("weights must be float32[M,224,224], got %s%s" % (w.dtype, w.shape))
        img_d = self._image_to_device(image)
        cls_d, k = self._classes_to_device(cls)

        def stage(s0, b):
            self.stage_soft_masks(img_d, torch.from_numpy(w[s0:s0 + b]).to(self.device), 0)

        scores, pred = self._score_classes_staged(int(w.shape[0]), stage, cls_d, k)
        return scores.cpu().numpy(), pred.cpu().numpy()

    def score_rise_classes(self, image, cells, shifts, s, classes):
        """score_rise for several classes of the same forwards: -> (scores f32[M,K], pred i32[M]); column i is
        score_rise(image, cells, shifts, s, classes[i])'s scores bit for bit.  classes: a sequence of class indices, or None for all."""
        cls = masks.class_selection(classes, None, NUM_CLASSES)[0]
        cells, shifts = masks.check_rise(cells, shifts, s)
        img_d = self._image_to_device(image)
        cells_d, shifts_d = torch.from_numpy(cells).to(self.device), torch.from_numpy(shifts).to(self.device)
        cls_d, k = self._classes_to_device(cls)

        def stage(s0, b):
            self.stage_rise(img_d, cells_d[s0:s0 + b], shifts_d[s0:s0 + b], s, 0)

        scores, pred = self._score_classes_staged(int(cells.shape[0]), stage, cls_d, k)
        return scores.cpu().numpy(), pred.cpu().numpy()

    def rise_saliency_classes(self, image, classes=None, top=None, n_masks=4000, s=7, p1=0.5, seed=0, out=None):
        """RISE's estimator as published, sal[k] = sum_m p_k(I * M_m) * M_m / (n_masks * p1): the maps of K classes from ONE pass over the
        masks of rise_saliency (masks.rise_masks(n_masks, s, p1, seed)).  -> (classes i32[K], sal f32[K,224,224]); map i is
        rise_saliency(image, classes[i], ...) bit for bit.  Exactly one of classes (a sequence of indices in [0, 1000)) and top (an int:
        the `top` largest logits of the unmasked forward, ties to the lower index) may be given; neither means all 1000 classes.
        Chunks of max_batch masks run apply -> forward -> class_scores -> rise_saliency_accumulate_classes on the stream with no host round
        trip in between.  out: None -> host arrays; a contiguous device f32[K,224,224] is overwritten with the maps and returned in
        their place (nothing is downloaded)."""
        cls, top = masks.class_selection(classes, top, NUM_CLASSES)
        if not 0.0 < float(p1) <= 1.0 or int(n_masks) <= 0:
            raise ValueError("n_masks > 0 and p1 in (0, 1], got n_masks=%r p1=%r" % (n_masks, p1))
        self._require_imagenet()
        cls = self._top_or_given(image, cls, top)
        cells, shifts = masks.rise_masks(n_masks, s, p1, seed)
        cls_d, k = self._classes_to_device(cls)
        sal = self._sal_out(out, k)
        img_d = self._image_to_device(image)
        cells_d, shifts_d = torch.from_numpy(cells).to(self.device), torch.from_numpy(shifts).to(self.device)

        def stage(s0, b):
            self.stage_rise(img_d, cells_d[s0:s0 + b], shifts_d[s0:s0 + b], s, 0)

        def after(s0, b, scores):
            self.rise_saliency_accumulate_classes(cells_d[s0:s0 + b], shifts_d[s0:s0 + b], s, scores, sal)

        self._score_classes_staged(int(n_masks), stage, cls_d, k, after=after)
        cls = np.arange(NUM_CLASSES, dtype=np.int32) if cls is None else cls
        return cls, self._sal_return(sal.div_(float(n_masks) * float(p1)), out)

    # ---- a linear surrogate over on/off superpixel rows (csrc/mpx_surrogate.h): LIME and KernelSHAP ----
    def surrogate_accumulate(self, onoff, weight, scores, A, B):
        """mpx_surrogate_accumulate: the fp64 moment sums of a weighted linear fit over on/off rows, in place, on the device.  With
        z~_m = (1, onoff[m] != 0), for m ascending: A[i][j] <- A[i][j] + weight[m] where z~_mi and z~_mj are on, B[i][k] <- B[i][k] +
        weight[m] * scores[m][k] where z~_mi is on; one fp64 rounding per step, masks.surrogate_sums bit for bit, however the rows are cut
        into calls.  onoff: device u8[M,S]; weight: device f32[M]; scores: device f32[M,K] (class_scores' output, rows >= K floats
        apart); A: device f64[S+1,S+1]; B: device f64[S+1,K].  Every engine takes it, the small networks included."""
        if onoff.device != self.device or onoff.dtype != torch.uint8 or onoff.dim() != 2 or not onoff.is_contiguous():
            raise ValueError("onoff must be a contiguous uint8[M,S] tensor on %s" % self.device)
        m, s = int(onoff.shape[0]), int(onoff.shape[1])
        if not 1 <= s <= _lib.SURROGATE_S_MAX:
            raise ValueError("S=%d outside [1, %d]" % (s, _lib.SURROGATE_S_MAX))
        if weight.device != self.device or weight.dtype != torch.float32 or tuple(weight.shape) != (m,) or not weight.is_contiguous():
            raise ValueError("weight must be a contiguous float32[%d] tensor on %s" % (m, self.device))
        if scores.dim() != 2 or B.dim() != 2:
            raise ValueError("scores must be float32[M,K] and B float64[S+1,K]")
        k = int(B.shape[1])
        if k < 1:
            raise ValueError("K >= 1, got B%s" % (tuple(B.shape),))
        pitch = self._class_score_rows(scores, m, k)
        for name, t, shape in (("A", A, (s + 1, s + 1)), ("B", B, (s + 1, k))):
            if t.device != self.device or t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float64[%d,%d] tensor on %s" % (name, shape[0], shape[1], self.device))
        _lib.check(self._h, self._lib.mpx_surrogate_accumulate(self._h, _ptr(onoff), _ptr(weight), _ptr(scores), pitch, m, s, k, _ptr(A),
                                                               _ptr(B), self._stream()), "mpx_surrogate_accumulate")
        return A, B

    def segment_paint(self, seg, value, out=None):
        """mpx_segment_paint: out[k][p] = value[k][seg[p]] on the device, +0.0 where seg[p] lies outside [0, S) (masks.segment_paint).
        seg: device i32[H,H] ranks, H = image_size; value: device f32[K,S] with unit column stride and rows >= S floats apart;
        out: None or a contiguous device f32[K,H,H], which is overwritten.  -> out."""
        h = self.image_size
        if seg.device != self.device or seg.dtype != torch.int32 or tuple(seg.shape) != (h, h) or not seg.is_contiguous():
            raise ValueError("seg must be a contiguous int32[%d,%d] tensor on %s" % (h, h, self.device))
        if value.dim() != 2 or value.shape[0] < 1:
            raise ValueError("value must be float32[K,S] with K >= 1")
        k, s = int(value.shape[0]), int(value.shape[1])
        if not 1 <= s <= _lib.SURROGATE_S_MAX:
            raise ValueError("S=%d outside [1, %d]" % (s, _lib.SURROGATE_S_MAX))
        pitch = self._class_score_rows(value, k, s, "value")
        if out is None:
            out = torch.empty(k, h, h, dtype=torch.float32, device=self.device)
        if out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != (k, h, h) or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32[%d,%d,%d] tensor on %s" % (k, h, h, self.device))
        _lib.check(self._h, self._lib.mpx_segment_paint(self._h, _ptr(seg), _ptr(value), pitch, s, k, _ptr(out), self._stream()),
                   "mpx_segment_paint")
        return out

    def _onoff_job(self, image, segments, onoff, stem):
        """What score_masks checks and uploads for ONE image's on/off rows -> (stage(s0, b), seg_d, onoff_d, M, S).  The staging rule is
        score_masks': the job's whole row count decides between table and conv (_staging); on the table path the table is built once."""
        self._require_imagenet()
        seg_rank, s = rank_segments(segments)
        onoff = self._host_onoff(onoff, s)
        m = int(onoff.shape[0])
        table = self._staging(stem, m) == "table"
        img_d = self._image_to_device(image)
        seg_d = torch.from_numpy(seg_rank).to(self.device)
        onoff_d = torch.from_numpy(onoff).to(self.device)

        def stage(s0, b):
            if table:
                if s0 == 0:
                    self.build_stem_table(img_d, seg_d, s)
                self.apply_stem_table(onoff_d[s0:s0 + b], 0)
            else:
                self.stage_masks(img_d, seg_d, onoff_d[s0:s0 + b], 0)

        return stage, seg_d, onoff_d, m, s

    def score_masks_classes(self, image, segments, onoff, classes, stem=None):
        """score_masks for several classes of the same forwards: -> (scores f32[M,K], pred i32[M]); column i is
        score_masks(image, segments, onoff, classes[i], stem=stem)'s scores bit for bit.  classes: a sequence of class indices, or None for
        all; stem as score_masks'."""
        cls = masks.class_selection(classes, None, NUM_CLASSES)[0]
        stage, _seg_d, _onoff_d, m, _s = self._onoff_job(image, segments, onoff, stem)
        cls_d, k = self._classes_to_device(cls)
        scores, pred = self._score_classes_staged(m, stage, cls_d, k)
        return scores.cpu().numpy(), pred.cpu().numpy()

    def _top_or_given(self, image, cls, top):
        """The classes of a many-class job as i32[K] or None (all): `top` = that many of the largest logits of the unmasked forward."""
        if top is None:
            return cls
        logits = self.score_masks(image, np.zeros((IMG, IMG), dtype=np.int32), np.ones((1, 1), dtype=np.uint8), 0, return_logits=True)[3]
        return masks.top_classes(logits[0], top)

    def _surrogate_job(self, image, segments, onoff, weight, cls, keep_rows, out):
        """The device half of lime / kernel_shap: chunks of max_batch rows run stage -> forward -> class_scores -> surrogate_accumulate on
        the stream with no host round trip in between, then ONE download of A, B and the class scores of the first keep_rows rows (fp32
        widened to fp64, which is exact).  `out` (None or the caller's device maps) is checked before anything runs.
        -> (A f64[S+1,S+1], B f64[S+1,K], rows f64[keep_rows,K], seg_d, S, K)."""
        stage, seg_d, onoff_d, m, s = self._onoff_job(image, segments, onoff, None)
        if not 1 <= s <= _lib.SURROGATE_S_MAX:
            raise ValueError("S=%d superpixels outside [1, %d]" % (s, _lib.SURROGATE_S_MAX))
        cls_d, k = self._classes_to_device(cls)
        if out is not None:
            self._sal_maps(out, k)
        n = s + 1
        buf = torch.zeros(n * n + n * k + keep_rows * k, dtype=torch.float64, device=self.device)
        a_d, b_d = buf[:n * n].view(n, n), buf[n * n:n * n + n * k].view(n, k)
        w_d = torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32)).to(self.device)

        def after(s0, b, scores):
            self.surrogate_accumulate(onoff_d[s0:s0 + b], w_d[s0:s0 + b], scores, a_d, b_d)

        scores, _pred = self._score_classes_staged(m, stage, cls_d, k, after=after)
        if keep_rows:
            buf[n * n + n * k:].view(keep_rows, k).copy_(scores[:keep_rows])
        host = buf.cpu().numpy()
        return (host[:n * n].reshape(n, n), host[n * n:n * n + n * k].reshape(n, k), host[n * n + n * k:].reshape(keep_rows, k),
                seg_d, s, k)

    def _paint_values(self, seg_d, values, out):
        """values f64[K,S] rounded to fp32, uploaded and painted -> host f32[K,224,224], or the device tensor `out` overwritten."""
        v_d = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(self.device)
        return self._sal_return(self.segment_paint(seg_d, v_d, out=out), out)

    def lime(self, image, segments, classes=None, top=None, n_samples=1000, kernel_width=0.25, lam=1.0, seed=0, out=None):
        """LIME on superpixels (Ribeiro et al., KDD 2016, in the lime_image form): a weighted ridge regression of K class scores on
        n_samples random on/off rows -- onoff = masks.lime_onoff(n_samples, S, seed), weight = masks.lime_weights(onoff, kernel_width).
        -> (classes i32[K], intercept f64[K], coef f64[K,S], sal f32[K,224,224]); coef[k][j] is the weight of the j-th superpixel in
        np.unique(segments) order, sal[k] paints the coefficients (rounded to fp32) onto the pixels.  classes / top as
        rise_saliency_classes.  The rows run at full batch (the stem table from stem_table_min_rows rows on) and their moment sums are
        accumulated on the device in fp64, in row order; the (S + 1)^2 solve is masks.lime_solve on the host, so the result is exactly
        lime_solve(surrogate_sums(score_masks_classes(...))).  out: None -> a host map; a contiguous device f32[K,224,224] is overwritten
        with the maps and returned in their place (nothing is downloaded)."""
        cls, top = masks.class_selection(classes, top, NUM_CLASSES)
        self._require_imagenet()
        if int(n_samples) < 1 or not float(lam) >= 0.0 or not float(kernel_width) > 0.0:
            raise ValueError("n_samples >= 1, lam >= 0 and kernel_width > 0, got %r, %r, %r" % (n_samples, lam, kernel_width))
        s = rank_segments(segments)[1]
        cls = self._top_or_given(image, cls, top)
        onoff = masks.lime_onoff(n_samples, s, seed)
        A, B, _rows, seg_d, s, k = self._surrogate_job(image, segments, onoff, masks.lime_weights(onoff, kernel_width), cls, 0, out)
        intercept, coef = masks.lime_solve(A, B, lam)
        cls = np.arange(NUM_CLASSES, dtype=np.int32) if cls is None else cls
        return cls, intercept, coef, self._paint_values(seg_d, coef, out)

    def kernel_shap(self, image, segments, classes=None, top=None, n_samples=2048, seed=0, out=None):
        """KernelSHAP on superpixels (Lundberg & Lee, NeurIPS 2017): the Shapley-kernel fit of K class scores on the rows [all off, all on]
        + masks.shap_onoff(n_samples, S, seed) with weights [0, 0, 1, ..] (a zero weight adds +0.0: the first two rows only bring f0 and
        f1), under phi_0 = f0 and sum(phi) = f1 - f0 (masks.shap_solve).  -> (classes i32[K], base f64[K] = f0, phi f64[K,S],
        sal f32[K,224,224]), phi indexed and painted as lime's coef.  ValueError for n_samples odd or below S, and for S < 2.  The device
        path, classes / top and out are lime's."""
        cls, top = masks.class_selection(classes, top, NUM_CLASSES)
        self._require_imagenet()
        s = rank_segments(segments)[1]
        if s < 2 or int(n_samples) % 2 or int(n_samples) < s:
            raise ValueError("S >= 2 and an even n_samples >= S, got S=%d n_samples=%r" % (s, n_samples))
        cls = self._top_or_given(image, cls, top)
        onoff = np.concatenate([np.zeros((1, s), np.uint8), np.ones((1, s), np.uint8), masks.shap_onoff(n_samples, s, seed)])
        weight = np.ones(onoff.shape[0], dtype=np.float32)
        weight[:2] = 0.0
        A, B, rows, seg_d, s, k = self._surrogate_job(image, segments, onoff, weight, cls, 2, out)
        phi = masks.shap_solve(A, B, rows[0], rows[1])
        cls = np.arange(NUM_CLASSES, dtype=np.int32) if cls is None else cls
        return cls, rows[0].copy(), phi, self._paint_values(seg_d, phi, out)

    # ---- a second pixel source (csrc/mpx_rankmask.h): rows selected on a per-pixel rank, the blurred image, the causal metrics ----
    def _chw_to_device(self, t, name):
        """A host or device f32[3,224,224] as a contiguous device tensor."""
        t = torch.as_tensor(t)
        if t.dtype != torch.float32 or tuple(t.shape) != (3, IMG, IMG):
            raise ValueError("%s must be float32[3,224,224], got %s%s" % (name, t.dtype, tuple(t.shape)))
        if t.is_cuda and t.device != self.device:
            raise ValueError("%s must be a host array or a tensor on %s" % (name, self.device))
        return t.contiguous().to(self.device)

    def blur_fill(self, image, taps=None, out=None):
        """mpx_blur_fill: -> device f32[3,224,224], the separable correlation of the normalised image with `taps` (host f32[klen], klen odd
        in [1, 31]; None = masks.gaussian_taps(), RISE's klen 11 and sigma 5), zero padding -- masks.blur_fill(x, taps) bit for bit.  image:
        u8[224,224,3] or normalised f32[3,224,224], host or device; out: a contiguous device f32[3,224,224] to write into (not the image)."""
        if self.small:
            raise ValueError("%s has no 224 x 224 input to blur" % self.arch)
        taps = masks.gaussian_taps() if taps is None else masks._check_taps(taps)
        img_d = self._image_to_device(image)
        if out is None:
            out = torch.empty(3, IMG, IMG, dtype=torch.float32, device=self.device)
        u8, f32 = self._soft_args(img_d, None, 0)
        if out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != (3, IMG, IMG) or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32[3,224,224] tensor on %s" % self.device)
        _lib.check(self._h, self._lib.mpx_blur_fill(self._h, u8, f32, taps.ctypes.data_as(C.POINTER(C.c_float)), int(taps.size), self._mean,
                                                    self._std, _ptr(out), self._stream()), "mpx_blur_fill")
        return out

    def stage_rank_masks(self, image, rank, thresh, fill=None, keep_top=False, slot0=0, out_f32=None):
        """mpx_rank_apply.  image as stage_masks; rank: device i32[224,224]; thresh: device i32[M]; fill: device f32[3,224,224] or None.
        Fills input slots [slot0, slot0+M): row m takes pixel p from the image where (rank[p] < thresh[m]) == keep_top and from `fill`
        elsewhere (None: image * 0.0, the binary masks' removed pixel) -- masks.rank_masks_apply bit for bit."""
        if rank.device != self.device or rank.dtype != torch.int32 or tuple(rank.shape) != (IMG, IMG) or not rank.is_contiguous():
            raise ValueError("rank must be a contiguous int32[224,224] tensor on %s" % self.device)
        if thresh.device != self.device or thresh.dtype != torch.int32 or thresh.dim() != 1 or not thresh.is_contiguous():
            raise ValueError("thresh must be a contiguous int32[M] tensor on %s" % self.device)
        if fill is not None and (fill.device != self.device or fill.dtype != torch.float32 or tuple(fill.shape) != (3, IMG, IMG)
                                 or not fill.is_contiguous()):
            raise ValueError("fill must be a contiguous float32[3,224,224] tensor on %s" % self.device)
        m = int(thresh.shape[0])
        u8, f32 = self._soft_args(image, out_f32, m)
        _lib.check(self._h, self._lib.mpx_rank_apply(self._h, u8, f32, _ptr(rank), _ptr(thresh), m, _ptr(fill), int(bool(keep_top)), self._mean,
                                                     self._std, int(slot0), _ptr(out_f32), self._stream()), "mpx_rank_apply")

    def score_rank_masks(self, image, rank, thresh, label, fill=None, keep_top=False, return_logits=False):
        """(image, rank i32[224,224], thresh i32[M], label) -> (score f32[M], pred i32[M][, logits f32[M,1000]]): the scores of the rows
        masks.rank_masks_apply(x, rank, thresh, fill, keep_top) describes, staged by mpx_rank_apply (always the conv staging).  fill: None
        or an f32[3,224,224], host or device.  Without a fill and with keep_top False, thresholds i * step give the scores of
        score_masks(..., stem="conv") over the pseudo-segments rank // step bit for bit."""
        rank, thresh = np.ascontiguousarray(rank), np.ascontiguousarray(thresh)
        if rank.dtype != np.int32 or rank.shape != (IMG, IMG):
            raise ValueError("rank must be int32[224,224], got %s%s" % (rank.dtype, rank.shape))
        if thresh.dtype != np.int32 or thresh.ndim != 1:
            raise ValueError("thresh must be int32[M], got %s%s" % (thresh.dtype, thresh.shape))
        self._require_imagenet()
        img_d = self._image_to_device(image)
        fill_d = None if fill is None else self._chw_to_device(fill, "fill")
        rank_d, thresh_d = torch.from_numpy(rank).to(self.device), torch.from_numpy(thresh).to(self.device)

        def stage(s0, b):
            self.stage_rank_masks(img_d, rank_d, thresh_d[s0:s0 + b], fill_d, keep_top, 0)

        return self._score_staged(int(thresh.shape[0]), stage, label, return_logits)

    def saliency_rank(self, sal):
        """masks.saliency_rank on the device: device f32[224,224] -> device i32[224,224], rank[p] = the position of pixel p in the stable
        sort by falling saliency (ties, +0.0 against -0.0 included, to the lower pixel index).  The key is 0 - sal, which is -sal with both
        zeros as +0.0, so that a sort that orders bit patterns cannot tell them apart.  A NaN or an infinity raises ValueError, as on
        the host (one flag is downloaded for it; the map is not)."""
        self._sal_map(sal)
        if not bool(torch.isfinite(sal).all()):
            raise ValueError("saliency holds a NaN or an infinity: its pixels have no order")
        order = torch.sort(0.0 - sal.flatten(), stable=True).indices
        rank = torch.empty(IMG * IMG, dtype=torch.int32, device=self.device)
        rank[order] = torch.arange(IMG * IMG, dtype=torch.int32, device=self.device)
        return rank.view(IMG, IMG)

    def _curve_fill(self, fill, img_d, taps, name):
        """One image's fill: None, "blur" (mpx_blur_fill of the image), or an f32[3,224,224]."""
        if fill is None:
            return None
        if isinstance(fill, str):
            if fill != "blur":
                raise ValueError('%s must be None, "blur" or a float32[3,224,224] image, got %r' % (name, fill))
            return self.blur_fill(img_d, taps)
        return self._chw_to_device(fill, name)

    def deletion_insertion_many(self, images, saliencies, labels, step=masks.CURVE_STEP, del_fill=None, ins_fill="blur", taps=None):
        """The deletion and the insertion curve (Petsiuk, Das, Saenko, BMVC 2018, section 4.1) of one saliency map per image -> a list of
        dicts {thresholds i32[T], del_scores / ins_scores f32[T], del_pred / ins_pred i32[T], del_auc, ins_auc}, T = ceil(50176 / step) + 1.
        Deletion row i replaces the thresholds[i] = min(i * step, 50176) most salient pixels by del_fill (None: zero, the binary masks'
        removed pixel); insertion row i shows them on ins_fill ("blur": mpx_blur_fill of the image with `taps`, None = masks.gaussian_taps()).
        A fill is None, "blur" or an f32[3,224,224] used for every image, or a list with one of these per image.  saliencies: host arrays
        or device f32[224,224] tensors (what rise_saliency(out=...) returns: nothing is downloaded in between); the ranks are
        masks.saliency_rank's.  The 2 T rows of consecutive images -- an image's deletion rows, then its insertion rows -- are packed into
        forwards of up to max_batch slots, one mpx_rank_apply per (image, curve, row range); all scores stay on the device until ONE
        download.  A row's bits depend neither on its slot nor on its neighbours: an image scores the same alone and packed."""
        self._require_imagenet()
        n = len(images)
        if not (len(saliencies) == len(labels) == n):
            raise ValueError("images, saliencies and labels must have the same length")
        fills = []
        for name, f in (("del_fill", del_fill), ("ins_fill", ins_fill)):
            per_image = isinstance(f, (list, tuple))
            if per_image and len(f) != n:
                raise ValueError("%s: a list needs one entry per image" % name)
            fills.append(list(f) if per_image else [f] * n)
        for lab in labels:
            if not 0 <= int(lab) < NUM_CLASSES:
                raise ValueError("label %r outside [0,1000)" % (lab,))
        if taps is not None:
            taps = masks._check_taps(taps)
        thresh = masks.curve_thresholds(step)
        t_rows = int(thresh.size)
        if n == 0:
            return []
        thresh_d = torch.from_numpy(thresh).to(self.device)
        total = 2 * t_rows * n
        label_rows = torch.from_numpy(np.repeat(np.asarray([int(v) for v in labels], dtype=np.int32), 2 * t_rows)).to(self.device)
        score = torch.empty(total, dtype=torch.float32, device=self.device)
        pred = torch.empty(total, dtype=torch.int32, device=self.device)
        pack = _Packer(self, label_rows, score, pred)
        for i in range(n):
            img_d = self._image_to_device(images[i])
            sal = saliencies[i]
            if isinstance(sal, torch.Tensor) and sal.is_cuda:
                rank_d = self.saliency_rank(sal)
            else:
                rank_d = torch.from_numpy(masks.saliency_rank(np.asarray(sal))).to(self.device)
            for keep_top, fill in ((False, self._curve_fill(fills[0][i], img_d, taps, "del_fill")),
                                   (True, self._curve_fill(fills[1][i], img_d, taps, "ins_fill"))):
                pack.add(t_rows, lambda r, take, slot0: self.stage_rank_masks(img_d, rank_d, thresh_d[r:r + take], fill, keep_top, slot0))
        pack.finish()
        score, pred = score.cpu().numpy().reshape(n, 2, t_rows), pred.cpu().numpy().reshape(n, 2, t_rows)
        return [{"thresholds": thresh.copy(),
                 "del_scores": score[i, 0].copy(), "ins_scores": score[i, 1].copy(),
                 "del_pred": pred[i, 0].copy(), "ins_pred": pred[i, 1].copy(),
                 "del_auc": masks.curve_auc(score[i, 0]), "ins_auc": masks.curve_auc(score[i, 1])} for i in range(n)]

    def deletion_insertion(self, image, saliency, label, step=masks.CURVE_STEP, del_fill=None, ins_fill="blur", taps=None):
        """deletion_insertion_many for one image: its deletion rows and its insertion rows go through the forward together."""
        return self.deletion_insertion_many([image], [saliency], [label], step=step, del_fill=del_fill, ins_fill=ins_fill, taps=taps)[0]

    # ---- Sobol total-order indices over a grid of cells (csrc/mpx_softmask.h DesignWeights): the design's rows gathered in the apply kernel ----
    def stage_sobol(self, image, A_d, B_d, grid, row0, m, slot0=0, out_f32=None, fill=None):
        """mpx_sobol_apply: rows [row0, row0 + m) of the total-order design (A_d, B_d: device f32[N, grid * grid]) into input slots
        [slot0, slot0 + m); the weights are masks.sobol_weights(A, B, grid, row0, m) bit for bit, gathered from the two matrices in the
        kernel.  fill: None (normalised image * w) or a device f32[3,224,224] F (fl(fl(v * w) + fl(F * fl(1 - w))): a cell is pulled
        towards F).  Values outside [0, 1] are the caller's contract (masks.check_sobol verifies host arrays before they are uploaded)."""
        d = int(grid)
        if not _lib.SOBOL_GRID_MIN <= d <= _lib.SOBOL_GRID_MAX:
            raise ValueError("grid=%r outside [%d, %d]" % (grid, _lib.SOBOL_GRID_MIN, _lib.SOBOL_GRID_MAX))
        for name, t in (("A_d", A_d), ("B_d", B_d)):
            if (t.device != self.device or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != d * d or t.shape[0] != A_d.shape[0]
                    or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32[N,%d] tensor on %s" % (name, d * d, self.device))
        if fill is not None and (fill.device != self.device or fill.dtype != torch.float32 or tuple(fill.shape) != (3, IMG, IMG)
                                 or not fill.is_contiguous()):
            raise ValueError("fill must be a contiguous float32[3,224,224] tensor on %s" % self.device)
        m = int(m)
        u8, f32 = self._soft_args(image, out_f32, m)
        _lib.check(self._h, self._lib.mpx_sobol_apply(self._h, u8, f32, _ptr(A_d), _ptr(B_d), int(A_d.shape[0]), d, int(row0), m, _ptr(fill),
                                                      self._mean, self._std, int(slot0), _ptr(out_f32), self._stream()), "mpx_sobol_apply")

    @staticmethod
    def _sobol_fill_arg(fill):
        """A driver's `fill`, checked on the host: None, "blur" or an f32[3,224,224] (host or device)."""
        if fill is None or (isinstance(fill, str) and fill == "blur"):
            return
        t = None if isinstance(fill, str) else torch.as_tensor(fill)
        if t is None or t.dtype != torch.float32 or tuple(t.shape) != (3, IMG, IMG):
            raise ValueError('fill must be None, "blur" or a float32[3,224,224] image, got %r'
                             % (fill if t is None else (t.dtype, tuple(t.shape)),))

    def _sobol_job(self, image, A, B, grid, fill, taps=None):
        """What the Sobol drivers check and upload -> (stage(s0, b), rows R, img_d): the design goes up once (2 N D floats), every chunk of
        rows is gathered from it by mpx_sobol_apply.  Everything is checked before anything touches the device."""
        self._require_imagenet()
        A, B = masks.check_sobol(A, B, grid)
        self._sobol_fill_arg(fill)
        if taps is not None:
            taps = masks._check_taps(taps)
        img_d = self._image_to_device(image)
        fill_d = self._curve_fill(fill, img_d, taps, "fill")
        a_d, b_d = torch.from_numpy(A).to(self.device), torch.from_numpy(B).to(self.device)

        def stage(s0, b):
            self.stage_sobol(img_d, a_d, b_d, grid, s0, b, 0, fill=fill_d)

        return stage, masks.sobol_rows(A.shape[0], grid), img_d

    def score_sobol(self, image, A, B, grid, label, fill=None, return_logits=False):
        """(image, A f32[N,D], B f32[N,D], grid, label) -> (score f32[R], pred i32[R][, logits f32[R,1000]]), R = N * (D + 1): the scores of
        the design's rows (masks.sobol_row_cells), whose weights masks.sobol_weights(A, B, grid, 0, R) are gathered in the apply kernel --
        score_soft_masks of those weights bit for bit, with 2 N D floats uploaded instead of 200 KB per row.  fill: None, "blur" or an
        f32[3,224,224] (stage_sobol)."""
        if not 0 <= int(label) < NUM_CLASSES:
            raise ValueError("label %r outside [0,1000)" % (label,))
        stage, rows, _img_d = self._sobol_job(image, A, B, grid, fill)
        return self._score_staged(rows, stage, label, return_logits)

    def score_sobol_classes(self, image, A, B, grid, classes, fill=None):
        """score_sobol for several classes of the same forwards: -> (scores f32[R,K], pred i32[R]); column i is
        score_sobol(image, A, B, grid, classes[i], fill)'s scores bit for bit.  classes: a sequence of class indices, or None for all."""
        cls = masks.class_selection(classes, None, NUM_CLASSES)[0]
        stage, rows, _img_d = self._sobol_job(image, A, B, grid, fill)
        cls_d, k = self._classes_to_device(cls)
        scores, pred = self._score_classes_staged(rows, stage, cls_d, k)
        return scores.cpu().numpy(), pred.cpu().numpy()

    def sobol_attribution(self, image, classes=None, top=None, grid=8, n_design=32, seed=0, fill=None, taps=None, out=None):
        """Sobol total-order indices of the cells of a grid x grid grid (Fel, Cadene, Chalvidal, Cord, Vigouroux, Serre, NeurIPS 2021): the
        share of each class score's variance that involves a cell, interactions included, from the R = n_design * (grid^2 + 1) rows of
        A, B = masks.sobol_design(n_design, grid, seed).  -> (classes i32[K], st f64[K,grid,grid], sal f32[K,224,224]);
        st = masks.sobol_total_order(score_sobol_classes(...), n_design) exactly, sal[k] paints st[k] (rounded to fp32) onto the cells.
        The design is uploaded once; chunks of max_batch rows run apply -> forward -> class_scores on the stream, the scores come down in
        ONE download and the estimator runs on the host in fp64.  fill: None (a cell is pulled towards zero), "blur" (towards
        blur_fill(image, taps), the paper's second perturbation) or an f32[3,224,224].  classes / top / out as rise_saliency_classes."""
        cls, top = masks.class_selection(classes, top, NUM_CLASSES)
        A, B = masks.sobol_design(n_design, grid, seed)
        d = int(grid)
        self._sobol_fill_arg(fill)
        self._require_imagenet()
        cls = self._top_or_given(image, cls, top)
        stage, rows, _img_d = self._sobol_job(image, A, B, d, fill, taps)
        cls_d, k = self._classes_to_device(cls)
        if out is not None:
            self._sal_maps(out, k)
        scores, _pred = self._score_classes_staged(rows, stage, cls_d, k)
        st = masks.sobol_total_order(scores.cpu().numpy(), n_design)
        seg_d = torch.from_numpy(masks.sobol_cell_map(d)).to(self.device)
        cls = np.arange(NUM_CLASSES, dtype=np.int32) if cls is None else cls
        return cls, st.reshape(k, d, d), self._paint_values(seg_d, st, out)

    # ---- occlusion sensitivity (csrc/mpx_softmask.h BoxWeights, csrc/mpx_occlusion.h): sliding boxes synthesised in the apply kernel ----
    def _boxes_d(self, boxes_d):
        if (boxes_d.device != self.device or boxes_d.dtype != torch.int32 or boxes_d.dim() != 2 or boxes_d.shape[1] != 4
                or not boxes_d.is_contiguous()):
            raise ValueError("boxes_d must be a contiguous int32[M,4] tensor on %s" % self.device)
        return int(boxes_d.shape[0])

    def stage_boxes(self, image, boxes_d, slot0=0, out_f32=None, fill=None):
        """mpx_box_apply: row m is the image with the box boxes_d[m] = (y0, x0, y1, x1) (device i32[M,4], half-open) covered, into input
        slots [slot0, slot0 + M); the weights are masks.box_weights(boxes) bit for bit, four compares per pixel in the kernel.  fill:
        None (a covered pixel is normalised image * 0.0: the mean colour) or a device f32[3,224,224] F (a covered pixel is F's).  The
        contract 0 <= y0 <= y1 <= 224, 0 <= x0 <= x1 <= 224 is the caller's (masks.check_boxes verifies host arrays before they are
        uploaded); the kernel never indexes by a box, so one outside it is memory-safe."""
        m = self._boxes_d(boxes_d)
        if fill is not None and (fill.device != self.device or fill.dtype != torch.float32 or tuple(fill.shape) != (3, IMG, IMG)
                                 or not fill.is_contiguous()):
            raise ValueError("fill must be a contiguous float32[3,224,224] tensor on %s" % self.device)
        u8, f32 = self._soft_args(image, out_f32, m)
        _lib.check(self._h, self._lib.mpx_box_apply(self._h, u8, f32, _ptr(boxes_d), m, _ptr(fill), self._mean, self._std, int(slot0),
                                                    _ptr(out_f32), self._stream()), "mpx_box_apply")

    def _box_job(self, image, boxes, fill, taps=None):
        """What the box drivers check and upload -> (stage(s0, b), rows M, boxes_d): the boxes go up once (16 bytes a row), every chunk
        of rows is synthesised from them by mpx_box_apply.  Everything is checked before anything touches the device."""
        self._require_imagenet()
        boxes = masks.check_boxes(boxes)
        self._sobol_fill_arg(fill)
        if taps is not None:
            taps = masks._check_taps(taps)
        img_d = self._image_to_device(image)
        fill_d = self._curve_fill(fill, img_d, taps, "fill")
        boxes_d = torch.from_numpy(boxes).to(self.device)

        def stage(s0, b):
            self.stage_boxes(img_d, boxes_d[s0:s0 + b], 0, fill=fill_d)

        return stage, int(boxes.shape[0]), boxes_d

    def score_boxes(self, image, boxes, label, fill=None, return_logits=False):
        """(image, boxes i32[M,4], label) -> (score f32[M], pred i32[M][, logits f32[M,1000]]): the scores of the image with one box
        covered per row -- score_soft_masks(image, masks.box_weights(boxes), label) bit for bit, with 16 bytes uploaded per row instead of
        200 KB.  fill: None, "blur" or an f32[3,224,224] (stage_boxes)."""
        if not 0 <= int(label) < NUM_CLASSES:
            raise ValueError("label %r outside [0,1000)" % (label,))
        stage, rows, _boxes_d = self._box_job(image, boxes, fill)
        return self._score_staged(rows, stage, label, return_logits)

    def score_boxes_classes(self, image, boxes, classes, fill=None):
        """score_boxes for several classes of the same forwards: -> (scores f32[M,K], pred i32[M]); column i is
        score_boxes(image, boxes, classes[i], fill)'s scores bit for bit.  classes: a sequence of class indices, or None for all."""
        cls = masks.class_selection(classes, None, NUM_CLASSES)[0]
        stage, rows, _boxes_d = self._box_job(image, boxes, fill)
        cls_d, k = self._classes_to_device(cls)
        scores, pred = self._score_classes_staged(rows, stage, cls_d, k)
        return scores.cpu().numpy(), pred.cpu().numpy()

    def _occlusion_maps(self, sum, cnt):
        if sum.dim() != 3:
            raise ValueError("sum must be float32[K,224,224]")
        k = int(sum.shape[0])
        self._sal_maps(sum, k)
        if cnt.device != self.device or cnt.dtype != torch.int32 or tuple(cnt.shape) != (IMG, IMG) or not cnt.is_contiguous():
            raise ValueError("cnt must be a contiguous int32[224,224] tensor on %s" % self.device)
        return k

    def occlusion_accumulate(self, boxes_d, scores, base, sum, cnt):
        """mpx_box_saliency_classes: for m ascending, on the pixels box m covers, sum[k][p] <- sum[k][p] + (base[k] - scores[m][k]) (a
        rounded subtraction and a rounded addition) and cnt[p] <- cnt[p] + 1, in place, on the device -- masks.occlusion_sums bit for bit,
        however the rows are cut into calls.  boxes_d: device i32[M,4]; scores: device f32[M,K] (class_scores' output, rows >= K floats
        apart); base: device f32[K], the scores of the whole image (it may be a row of the tensor scores is a view of); sum: device
        f32[K,224,224]; cnt: device i32[224,224]."""
        m = self._boxes_d(boxes_d)
        k = self._occlusion_maps(sum, cnt)
        if scores.dim() != 2:
            raise ValueError("scores must be float32[M,K]")
        pitch = self._class_score_rows(scores, m, k)
        if base.device != self.device or base.dtype != torch.float32 or tuple(base.shape) != (k,) or not base.is_contiguous():
            raise ValueError("base must be a contiguous float32[%d] tensor on %s" % (k, self.device))
        if m == 0:              # an empty tensor has no pointer to hand over, and there is nothing to add
            return sum, cnt
        _lib.check(self._h, self._lib.mpx_box_saliency_classes(self._h, _ptr(boxes_d), _ptr(scores), pitch, _ptr(base), m, k, _ptr(sum),
                                                               _ptr(cnt), self._stream()), "mpx_box_saliency_classes")
        return sum, cnt

    def occlusion_mean(self, sum, cnt, out=None):
        """mpx_box_saliency_mean: out[k][p] = sum[k][p] / float(cnt[p]) where cnt[p] > 0 (one rounded division), 0.0 elsewhere --
        masks.occlusion_mean bit for bit.  out: None (a new device f32[K,224,224]) or a contiguous device f32[K,224,224]; it may be sum."""
        k = self._occlusion_maps(sum, cnt)
        if out is None:
            out = torch.empty(k, IMG, IMG, dtype=torch.float32, device=self.device)
        self._sal_maps(out, k)
        _lib.check(self._h, self._lib.mpx_box_saliency_mean(self._h, _ptr(sum), _ptr(cnt), k, _ptr(out), self._stream()),
                   "mpx_box_saliency_mean")
        return out

    def occlusion(self, image, classes=None, top=None, window=32, stride=16, fill=None, taps=None, out=None):
        """Occlusion sensitivity (Zeiler, Fergus, ECCV 2014): a window x window box slides over the image by `stride`
        (masks.occlusion_boxes; ints, (h, w) pairs, or a list of (window, stride) scales), and every pixel gets the mean, over the R boxes
        that cover it, of the drop of the class score from the whole image to the image with the box covered.
        -> (classes i32[K], base f32[K], scores f32[R,K], sal f32[K,224,224]): base the whole image's scores, scores[r] the scores under
        box r, sal = masks.occlusion_mean(*masks.occlusion_sums(0, 0, boxes, scores, base)) bit for bit.  The job is the empty box, then
        the R boxes: its row 0 is base.  The boxes are uploaded once; chunks of max_batch rows run apply -> forward -> class_scores on the
        stream, then one mpx_box_saliency_classes over rows 1 .. R and one mpx_box_saliency_mean, with no download before the end.
        fill: None (the box is the mean colour), "blur" (blur_fill(image, taps)) or an f32[3,224,224].  classes / top as
        rise_saliency_classes.  out: None -> host arrays; a contiguous device f32[K,224,224] is overwritten with the maps and returned in
        their place, and base and scores are returned as device tensors (nothing is downloaded)."""
        cls, top = masks.class_selection(classes, top, NUM_CLASSES)
        boxes = np.concatenate([np.zeros((1, 4), dtype=np.int32), masks.occlusion_boxes(window, stride)])
        self._sobol_fill_arg(fill)
        self._require_imagenet()
        cls = self._top_or_given(image, cls, top)
        stage, rows, boxes_d = self._box_job(image, boxes, fill, taps)
        cls_d, k = self._classes_to_device(cls)
        sal = self._sal_out(out, k)
        cnt = torch.zeros(IMG, IMG, dtype=torch.int32, device=self.device)
        scores, _pred = self._score_classes_staged(rows, stage, cls_d, k)
        self.occlusion_accumulate(boxes_d[1:], scores[1:], scores[0], sal, cnt)
        self.occlusion_mean(sal, cnt, out=sal)
        cls = np.arange(NUM_CLASSES, dtype=np.int32) if cls is None else cls
        if out is not None:
            return cls, scores[0], scores[1:], sal
        host = scores.cpu().numpy()
        return cls, host[0], host[1:], sal.cpu().numpy()

    # ---- Score-CAM (csrc/mpx_softmask.h MapWeights, csrc/mpx_cam.h): the network's own activation maps as masks ----
    def pool_input(self, slot=0):
        """mpx_pool_input + mpx_planes_to_chw: device f32[C,g,g], the map the global average pool read for row `slot` of the LAST forward,
        as the pool saw it (its ReLU6 / SiLU on load applied), logical channels only -- Score-CAM's and CAM's default target layer (ResNet's
        layer4, MobileNetV2's features.18, SqueezeNet's classifier map of 1000 channels ...).  ValueError for a slot the last forward did
        not run; MpxError (MPX_E_STATE) on a network without such a pool (the VGGs, AlexNet, ViT, the small networks)."""
        hi, lo = C.c_void_p(), C.c_void_p()
        side, ch, pitch, load = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(self._h, self._lib.mpx_pool_input(self._h, C.byref(hi), C.byref(lo), C.byref(side), C.byref(ch), C.byref(pitch),
                                                     C.byref(load)), "mpx_pool_input")
        if isinstance(slot, bool) or int(slot) != slot or not 0 <= int(slot) < self._last_batch:
            raise ValueError("pool_input: slot %r outside the last forward's [0, %d)" % (slot, self._last_batch))
        out = torch.empty(ch.value, side.value, side.value, dtype=torch.float32, device=self.device)
        _lib.check(self._h, self._lib.mpx_planes_to_chw(self._h, hi, lo, int(slot), side.value, ch.value, pitch.value, load.value, _ptr(out),
                                                        self._stream()), "mpx_planes_to_chw")
        return out

    def _cam_maps(self, t, name):
        """A contiguous device f32[N,g,g] with 2 <= g <= 16 -> (N, g)."""
        if (t.device != self.device or t.dtype != torch.float32 or t.dim() != 3 or t.shape[1] != t.shape[2] or not t.is_contiguous()
                or not masks.CAM_GRID_MIN <= int(t.shape[1]) <= masks.CAM_GRID_MAX):
            raise ValueError("%s must be a contiguous float32[N,g,g] tensor on %s with g in [%d, %d]"
                             % (name, self.device, masks.CAM_GRID_MIN, masks.CAM_GRID_MAX))
        return int(t.shape[0]), int(t.shape[1])

    def cam_cells(self, act_d):
        """mpx_cam_cells: act_d device f32[C,g,g] -> (cells f32[C,g,g], lo f32[C], hi f32[C], valid u8[C]) on the device --
        masks.cam_cells bit for bit: every channel normalised by the extremes of its UPSAMPLED map; a flat channel is invalid, cells +0.0."""
        c, g = self._cam_maps(act_d, "act_d")
        cells = torch.empty_like(act_d)
        lo = torch.empty(c, dtype=torch.float32, device=self.device)
        hi = torch.empty(c, dtype=torch.float32, device=self.device)
        valid = torch.empty(c, dtype=torch.uint8, device=self.device)
        if c:
            _lib.check(self._h, self._lib.mpx_cam_cells(self._h, _ptr(act_d), c, g, _ptr(cells), _ptr(lo), _ptr(hi), _ptr(valid),
                                                        self._stream()), "mpx_cam_cells")
        return cells, lo, hi, valid

    def stage_cam(self, image, cells_d, slot0=0, out_f32=None):
        """mpx_cam_apply: row m is the image times min(max(up(cells_d[m]), 0), 1) (cells_d device f32[M,g,g], upsampled to 224 x 224 in
        the kernel), into input slots [slot0, slot0 + M); the weights are masks.cam_weights(cells) bit for bit."""
        m, g = self._cam_maps(cells_d, "cells_d")
        u8, f32 = self._soft_args(image, out_f32, m)
        _lib.check(self._h, self._lib.mpx_cam_apply(self._h, u8, f32, _ptr(cells_d), m, g, self._mean, self._std, int(slot0), _ptr(out_f32),
                                                    self._stream()), "mpx_cam_apply")

    def _cam_job(self, image, cells):
        """What the row scorers check and upload -> (stage(s0, b), rows M): the cells go up once (g * g floats a row)."""
        self._require_imagenet()
        cells = np.ascontiguousarray(cells)
        if (cells.dtype != np.float32 or cells.ndim != 3 or cells.shape[1] != cells.shape[2]
                or not masks.CAM_GRID_MIN <= cells.shape[1] <= masks.CAM_GRID_MAX or not np.isfinite(cells).all()):
            raise ValueError("cells must be finite float32[M,g,g] with g in [%d, %d], got %s%s"
                             % (masks.CAM_GRID_MIN, masks.CAM_GRID_MAX, cells.dtype, cells.shape))
        img_d = self._image_to_device(image)
        cells_d = torch.from_numpy(cells).to(self.device)

        def stage(s0, b):
            self.stage_cam(img_d, cells_d[s0:s0 + b], 0)

        return stage, int(cells.shape[0])

    def score_cam_rows(self, image, cells, label, return_logits=False):
        """(image, cells f32[M,g,g], label) -> (score f32[M], pred i32[M][, logits f32[M,1000]]): the scores of the image under the
        upsampled maps -- score_soft_masks(image, masks.cam_weights(cells), label) bit for bit, with g * g floats uploaded per row instead
        of 200 KB."""
        if not 0 <= int(label) < NUM_CLASSES:
            raise ValueError("label %r outside [0,1000)" % (label,))
        stage, rows = self._cam_job(image, cells)
        return self._score_staged(rows, stage, label, return_logits)

    def score_cam_rows_classes(self, image, cells, classes):
        """score_cam_rows for several classes of the same forwards: -> (scores f32[M,K], pred i32[M]); column i is
        score_cam_rows(image, cells, classes[i])'s scores bit for bit.  classes: a sequence of class indices, or None for all."""
        cls = masks.class_selection(classes, None, NUM_CLASSES)[0]
        stage, rows = self._cam_job(image, cells)
        cls_d, k = self._classes_to_device(cls)
        scores, pred = self._score_classes_staged(rows, stage, cls_d, k)
        return scores.cpu().numpy(), pred.cpu().numpy()

    def cam_combine(self, act_d, scores, low=None, out=None):
        """mpx_cam_combine: (low f32[K,g,g], sal f32[K,224,224]) on the device -- masks.cam_combine bit for bit: low[k] = the sum over the
        rows r, in order, of scores[r][k] * act_d[r] (a rounded product and a rounded sum per step, the RAW activations), sal[k] =
        relu(up(low[k])).  act_d: device f32[R,g,g]; scores: device f32[R,K] (class_scores' output, rows >= K floats apart); low / out:
        None or contiguous device f32[K,g,g] / f32[K,224,224], overwritten.  R = 0 gives zero maps."""
        r, g = self._cam_maps(act_d, "act_d")
        if scores.dim() != 2 or scores.shape[1] < 1:
            raise ValueError("scores must be float32[R,K] with K >= 1")
        k = int(scores.shape[1])
        pitch = self._class_score_rows(scores, r, k)
        if low is None:
            low = torch.empty(k, g, g, dtype=torch.float32, device=self.device)
        if low.device != self.device or low.dtype != torch.float32 or tuple(low.shape) != (k, g, g) or not low.is_contiguous():
            raise ValueError("low must be a contiguous float32[%d,%d,%d] tensor on %s" % (k, g, g, self.device))
        if out is None:
            out = torch.empty(k, IMG, IMG, dtype=torch.float32, device=self.device)
        self._sal_maps(out, k)
        _lib.check(self._h, self._lib.mpx_cam_combine(self._h, _ptr(act_d) if r else None, _ptr(scores) if r else None, pitch, r, g, k,
                                                      _ptr(low), _ptr(out), self._stream()), "mpx_cam_combine")
        return low, out

    def score_cam(self, image, classes=None, top=None, activations=None, out=None):
        """Score-CAM (Wang et al., CVPR-W 2020): every channel of the map the global pool reads is upsampled to the image, normalised to
        [0, 1] and scored as a mask; the class activation map is the channels' sum weighted by those scores.
        -> (classes i32[K], channels i32[R], scores f32[R,K], low f32[K,g,g], sal f32[K,224,224]): channels the R channels that are not
        flat (a flat one is skipped, as published), scores[r][k] the softmax probability of class k under channel channels[r]'s mask,
        (low, sal) = masks.cam_combine(act[channels], scores) bit for bit -- low the map at layer resolution, sal = relu(up(low)) before
        the caller's min-max.  ONE unmasked forward (staged through the box entry with the empty box) gives the logits behind top= and the
        tap pool_input(0); activations= (f32[C,g,g], e.g. from a torch hook) replaces the tap -- the only way on a network without a
        global pool.  valid comes down (C bytes), the valid channels are compacted with a torch index, chunks of max_batch rows run apply ->
        forward -> class_scores on the stream, then one mpx_cam_combine; one download at the end.  classes / top as rise_saliency_classes.
        out: None -> host arrays; a contiguous device f32[K,224,224] is overwritten with the maps and returned in their place, and
        scores and low are returned as device tensors (nothing further is downloaded)."""
        cls, top = masks.class_selection(classes, top, NUM_CLASSES)
        self._require_imagenet()
        if activations is not None:
            activations = masks.check_activations(activations)
        img_d = self._image_to_device(image)
        if top is not None or activations is None:
            labels = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.stage_boxes(img_d, torch.zeros(1, 4, dtype=torch.int32, device=self.device), 0)
            logits = self.forward(1, labels, want_logits=True)[2]
            if activations is None:
                act_d = self.pool_input(0)
            if top is not None:
                cls = masks.top_classes(logits[0].cpu().numpy(), top)
        if activations is not None:
            act_d = torch.from_numpy(activations).to(self.device)
        cls_d, k = self._classes_to_device(cls)
        if out is not None:
            self._sal_maps(out, k)
        cells_d, _lo, _hi, valid = self.cam_cells(act_d)
        keep = torch.nonzero(valid.cpu()).reshape(-1)                  # C bytes come down; the compaction is a torch index
        keep_d = keep.to(self.device)
        cells_d, act_d = cells_d[keep_d].contiguous(), act_d[keep_d].contiguous()
        rows = int(keep.numel())

        def stage(s0, b):
            self.stage_cam(img_d, cells_d[s0:s0 + b], 0)

        scores, _pred = self._score_classes_staged(rows, stage, cls_d, k)
        low, sal = self.cam_combine(act_d, scores, out=out)
        cls = np.arange(NUM_CLASSES, dtype=np.int32) if cls is None else cls
        channels = keep.numpy().astype(np.int32)
        if out is not None:
            return cls, channels, scores, low, sal
        return cls, channels, scores.cpu().numpy(), low.cpu().numpy(), sal.cpu().numpy()

    # ---- kernel variants (tuning / tests) ----
    def set_conv_tile(self, layer, tile):
        """Select the conv kernel variant of one layer (index or torchvision name); tile < 0 = default."""
        i = layer if isinstance(layer, int) else [d.name.decode() for d in self.layers].index(layer)
        _lib.check(self._h, self._lib.mpx_set_conv_tile(self._h, int(i), int(tile)), "mpx_set_conv_tile")

    def set_fusion(self, on=True):
        """mpx_set_fusion.  True (default state) = every fusion: a stage's first conv3 with its downsample conv as one
        K-concatenated launch, the ImageNet stem with its max pool, layer1's block tails (conv2 -> conv3 + identity -> the
        next block's conv1, mpx_bottleneck_tail) and layer2's pointwise tails (conv3 + identity -> the next block's conv1,
        mpx_pointwise_tail).  False = one launch per layer.  An int is passed through as the mask (1 = round 2's fusions
        without the tails, 3 = without the pointwise tails).  The stem fusion is bit-identical to the separate launches; the
        others change the fp32 summation order (same tolerance)."""
        mask = (7 if on else 0) if isinstance(on, bool) else int(on)
        _lib.check(self._h, self._lib.mpx_set_fusion(self._h, mask), "mpx_set_fusion")

    def bottleneck_tails(self):
        """[(conv2, conv3, downsample or -1, next conv1)] layer indices of the blocks whose tail runs as one launch."""
        out = []
        for k in range(self._lib.mpx_num_bottleneck_tails(self._h)):
            v = [C.c_int() for _ in range(4)]
            _lib.check(self._h, self._lib.mpx_bottleneck_tail_info(self._h, k, *[C.byref(x) for x in v]), "mpx_bottleneck_tail_info")
            out.append(tuple(int(x.value) for x in v))
        return out

    def pointwise_tails(self):
        """[(conv3, next conv1)] layer indices of the pairs that run as one pointwise-tail launch."""
        out = []
        for k in range(self._lib.mpx_num_pointwise_tails(self._h)):
            v = [C.c_int() for _ in range(2)]
            _lib.check(self._h, self._lib.mpx_pointwise_tail_info(self._h, k, *[C.byref(x) for x in v]), "mpx_pointwise_tail_info")
            out.append(tuple(int(x.value) for x in v))
        return out

    def conv_tile(self, layer):
        i = layer if isinstance(layer, int) else [d.name.decode() for d in self.layers].index(layer)
        return int(self._lib.mpx_get_conv_tile(self._h, int(i)))

    # ---- profiling ----
    def profile(self, on=True):
        _lib.check(self._h, self._lib.mpx_profile_enable(self._h, 1 if on else 0), "mpx_profile_enable")

    def collect_profile(self):
        """{'ms': {kind: ms}, 'launches': {kind: n}, 'per_conv_ms': [...], 'per_norm_ms': [...], 'avgpool2_ms': ms} accumulated since the
        last call.  per_norm_ms (one entry per stand-alone BatchNorm: its concat-append + BN + ReLU launch) and avgpool2_ms (the
        transitions' average pools) split what a DenseNet engine books under 'pool'; empty / 0 on every other architecture.  'per_dw_ms'
        (one entry per depthwise layer) is the same split on a MobileNetV2 engine, 'per_clip_pool_ms' (one entry per clipped 3x3 max pool,
        mpx_clip_pool_info) on a GoogLeNet engine, 'per_shuffle_ms' (one entry per channel shuffle, mpx_shuffle_info) on a ShuffleNetV2 engine,
        'per_se_gate_ms' / 'per_se_scale_ms' (one entry per SE layer: its gate and its scale launch) on an EfficientNet-B0 engine,
        'per_lnorm_ms' (one entry per stand-alone LayerNorm, mpx_lnorm_info; the depthwise + LayerNorm launches are per_dw_ms's) on a
        ConvNeXt engine, 'per_attn_ms' (one entry per attention launch, mpx_attn_info) and 'tokens_ms' (the token assembly) on a ViT engine,
        whose LayerNorms are per_lnorm_ms's."""
        ms = (C.c_double * 4)()
        n = (C.c_longlong * 4)()
        per = (C.c_double * len(self.layers))()
        per_norm = (C.c_double * max(1, len(self.norms)))()
        avg2 = (C.c_double * 1)()
        per_dw = (C.c_double * max(1, len(self.dwconvs)))()
        n_cp = int(self._lib.mpx_num_clip_pools(self._h))
        per_cp = (C.c_double * max(1, n_cp))()
        n_sh = int(self._lib.mpx_num_shuffles(self._h))
        per_sh = (C.c_double * max(1, n_sh))()
        per_sg = (C.c_double * max(1, len(self.ses)))()
        per_ss = (C.c_double * max(1, len(self.ses)))()
        per_ln = (C.c_double * max(1, len(self.lnorms)))()
        per_at = (C.c_double * max(1, len(self.attns)))()
        tok = (C.c_double * 1)()
        _lib.check(self._h, self._lib.mpx_profile_collect_attn(self._h, ms, n, per, per_norm, avg2, per_dw, per_cp, per_sh, per_sg, per_ss, per_ln, per_at, tok),
                   "mpx_profile_collect_attn")
        kinds = ("conv", "mask_apply_normalize", "pool", "head")
        return {"ms": dict(zip(kinds, list(ms))), "launches": dict(zip(kinds, list(n))),
                "per_conv_ms": list(per), "per_norm_ms": list(per_norm)[:len(self.norms)], "avgpool2_ms": float(avg2[0]),
                "per_dw_ms": list(per_dw)[:len(self.dwconvs)], "per_clip_pool_ms": list(per_cp)[:n_cp], "per_shuffle_ms": list(per_sh)[:n_sh],
                "per_se_gate_ms": list(per_sg)[:len(self.ses)], "per_se_scale_ms": list(per_ss)[:len(self.ses)],
                "per_lnorm_ms": list(per_ln)[:len(self.lnorms)], "per_attn_ms": list(per_at)[:len(self.attns)], "tokens_ms": float(tok[0])}
