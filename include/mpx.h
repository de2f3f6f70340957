/* mpx.h -- C-ABI of the MI355X masked-perturbation scoring engine ("mpx").
 *
 * Drop-in boundary for ONE path of LiliMeng/network_interpretation_imagenet: for one
 * 224x224 image, apply M superpixel on/off mask-vectors to the normalised image, run one
 * ResNet forward per mask, return softmax(logits)[label] and argmax(logits) per mask.
 * The reference has no FFI layer (it is 100 % Python); every entry point below names the
 * reference lines it replaces.  Paths are relative to the reference repository root.
 *
 * Conventions
 *   - Plain C types only.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - Pointers marked DEV are device pointers owned by the caller; HOST are host pointers.
 *     The engine never frees or retains caller memory; it owns only its workspace.
 *   - Every function returns 0 on success, a positive hipError_t, or a negative MPX_E_* code,
 *     never throws, never exits, and (unless stated) does not synchronise the stream.
 *   - Activations between kernels live in HBM as TWO fp16 planes in NHWC order ("split-fp16":
 *     x ~= hi + lo, 22 significant bits, 4 bytes per element like fp32).  Convolutions run on
 *     the fp16 MFMA pipe as hi*hi + hi*lo + lo*hi with fp32 accumulation.
 *   - One engine per process per GPU.  Calls on one engine must not overlap from two threads.
 */
#ifndef MPX_H
#define MPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPX_IMG 224          /* n = 224, generate_gp_training_data_imagenet.py:84-88 */
#define MPX_IMG_PAD 230      /* 3-pixel zero border, the 7x7 stem's padding=3, stored explicitly */
#define MPX_NUM_CLASSES 1000

enum {
    MPX_E_ARG = -1,      /* bad argument (null pointer, shape, range) */
    MPX_E_STATE = -2,    /* weights missing, batch larger than max_batch, ... */
    MPX_E_NOMEM = -3,
    MPX_E_INTERNAL = -4
};

/* arch_id = the torchvision ResNet depth the reference selects with `-a` / `--arch`
 * (generate_gp_training_data_imagenet.py:45,579): 18, 34, 50, 101 or 152 -- or one of the reference's two small networks
 * (SURVEY.md 8 f4), whose trained checkpoints ship with it:
 *   MPX_ARCH_MNIST_NET            Classification_Net, 28x28x1 -> 10 (generate_gp_training_data_mnist.py:86-105)
 *   MPX_ARCH_CIFAR_RESNET + depth ResNetCifar(depth = 6n+2), 32x32x3 -> 10 (models/resnet.py:77-146; the checkpoint is depth 56)
 * -- or one of torchvision's VGG networks, which the reference's `-a` also selects (its README lists them next to the ResNets):
 *   MPX_ARCH_VGG + depth          vgg11 / vgg13 / vgg16 / vgg19 (torchvision cfgs A / B / D / E), depth 11, 13, 16 or 19
 *   MPX_ARCH_VGG_BN + depth       the same with BatchNorm2d after every conv (vgg11_bn ... vgg19_bn)
 * A VGG engine is a plain chain: 3x3 conv (+ bias, + BN) + ReLU layers with 2x2 stride-2 max pools (mpx_maxpool2x2s2), then the classifier
 * as three more entries of the conv list (classifier.0 = a 7x7 valid conv over the [B][7][7][512] map, K = 25088; classifier.3 = 1x1
 * 4096 -> 4096; classifier.6 = the logit layer).  AdaptiveAvgPool2d((7, 7)) is the identity at 224 input and Dropout is the identity in
 * eval, so neither is an op.  It stages through mpx_mask_apply_normalize only: it has no 7x7 stem, so the stem-table and stem + pool
 * entry points return MPX_E_STATE.  Its first layer (3 -> 64, 3x3 pad 1) reads the padded NHWC4 staging as the ResNet stem does.
 * -- or torchvision's AlexNet, the third family the reference's README names for `-a`:
 *   MPX_ARCH_ALEXNET              alexnet (any other id in [4000, 4100) is MPX_E_ARG)
 * An AlexNet engine is a plain chain too: features.0 (3 -> 64, 11x11 stride 4 pad 2, 224 -> 55), features.3 (64 -> 192, 5x5 pad 2, 27x27),
 * features.6 / .8 / .10 (192 -> 384 -> 256 -> 256, 3x3 pad 1, 13x13), each with bias + ReLU, three 3x3 stride-2 max pools WITHOUT padding
 * (mpx_maxpool3x3s2p0: 55 -> 27 -> 13 -> 6), then classifier.1 = a 6x6 valid conv over the [B][6][6][256] map (K = 9216), classifier.4 =
 * 1x1 4096 -> 4096, classifier.6 = the logit layer.  AdaptiveAvgPool2d((6, 6)) is the identity at 224 input.  Two activation buffers of
 * 55 * 55 * 64 elements per image (2.4 MB per slot with the staging).  Like VGG it stages through mpx_mask_apply_normalize only and the
 * stem-table and stem + pool entry points return MPX_E_STATE.  features.0 reads the padded NHWC4 staging, one run of 16 pixels x 4
 * channels (two K steps) per kernel row: k_packed = 11 * 64 = 704.
 * -- or one of torchvision's DenseNets with growth rate 32, the last classic family the reference's `-a` reaches (it also carries one of its
 * own: models/densenet.py):
 *   MPX_ARCH_DENSENET + depth     densenet121 / densenet169 / densenet201 (block sizes (6, 12, 24, 16) / (6, 12, 32, 32) / (6, 12, 48, 32));
 *                                 any other id in [5000, 6000) is MPX_E_ARG (densenet161 -- growth rate 48, 96 initial features -- included)
 * A DenseNet engine runs the ResNet stem shape (features.conv0 3 -> 64 7x7 stride 2 + norm0 + ReLU + MaxPool(3, 2, 1): the fused stem + pool
 * launch), then four dense blocks.  A dense layer is norm1 -> ReLU -> conv1 (1x1, C -> 128) -> norm2 -> ReLU -> conv2 (3x3 pad 1, 128 -> 32),
 * its 32 channels concatenated behind its C input channels.  BatchNorm + ReLU sit BEFORE conv1, and every later layer normalises the same
 * concatenation with statistics of its own, so they cannot ride in a producer's epilogue: the engine keeps the block's concatenation raw
 * ([B][H][W][C_block], channel-strided) and runs mpx_concat_bn_relu once per dense layer -- it appends conv2's output to the concatenation and
 * writes relu(bn(.)) of the first C channels as the dense operand of the next conv1 / transition conv / the head.  norm2 + ReLU are conv1's
 * epilogue; conv2 has neither BatchNorm nor ReLU nor bias.  A transition is norm -> ReLU -> conv (1x1, C -> C / 2, no bias) ->
 * mpx_avgpool2x2s2; the head is norm5 -> ReLU -> mpx_global_avgpool -> classifier (Linear(C_final, 1000), the logit layer).  The
 * stand-alone BatchNorms (every norm1, each transition's norm, norm5) belong to no conv: mpx_num_norms / mpx_norm_info / mpx_load_norm.
 * Four ResNet-sized activation buffers (14.5 MB per slot with the staging and the pooled stem planes).  It stages through
 * mpx_mask_apply_normalize only: the stem-table entry points return MPX_E_STATE.
 * -- or torchvision's MobileNetV2 (width 1.0), the first mobile network of `models.__dict__[arch]` the engine serves:
 *   MPX_ARCH_MOBILENET + 2        mobilenet_v2; every other id in [6000, 7000) is MPX_E_ARG
 * A MobileNetV2 engine runs features.0 (3 -> 32, 3x3 stride 2 pad 1, reading the padded NHWC4 staging: k_packed = 96) + BN + ReLU6, 17
 * inverted-residual blocks (t, c, n, s) = (1,16,1,1) (6,24,2,2) (6,32,3,2) (6,64,4,2) (6,96,3,1) (6,160,3,2) (6,320,1,1) -- 1x1 expand + BN +
 * ReLU6 (absent when t = 1), depthwise 3x3 + BN + ReLU6 (mpx_dwconv3x3_bn_relu6), 1x1 project + BN without activation, plus the block input
 * when stride is 1 and cin == cout (the residual operand of the project conv; no ReLU behind the add) --, features.18 (320 -> 1280, 1x1) + BN +
 * ReLU6, mpx_global_avgpool_clamp6 and classifier.1 (Linear(1280, 1000), the logit layer).  The 1x1 and stem convs are entries of the conv
 * list; the 17 depthwise layers are a list of their own: mpx_num_dwconvs / mpx_dwconv_info / mpx_load_dwconv.
 * THE CLAMP BELONGS TO THE CONSUMER.  The MFMA conv kernels' epilogues know ReLU only, and relu6(x) = min(relu(x), 6): a conv that torchvision
 * follows with ReLU6 (relu = 1 in its descriptor: the stem, every expand conv, features.18) stores the ReLU output, and whoever reads it takes
 * min(x, 6) as it loads -- a depthwise layer (clamp_in = 1) or the clamped global pool.  mpx_conv_bn_act on such a layer therefore returns
 * relu(bn(conv(x))), NOT relu6(.); mpx_conv_desc keeps its layout.  The depthwise kernel applies its own full ReLU6.
 * Channel counts 16, 24 and 144 are stored with a pitch of 32, 32 and 160 (k_packed = ksize^2 * pitch of the input, zero weight columns, zero
 * scale and shift on the padded rows: padded channels are exact zeros wherever they are read); such layers run the generic tiles only.
 * Three activation buffers of 112 * 112 * 96 elements per image (features.2's expanded map, 1.5 x a ResNet buffer): 15.3 MB per slot with
 * the staging.  It stages through mpx_mask_apply_normalize only: the stem-table and stem + pool entry points return MPX_E_STATE.
 * -- or torchvision's SqueezeNet 1.1, the small network of the model zoo (1.2 M parameters, 0.35 GMAC per forward):
 *   MPX_ARCH_SQUEEZENET + 11      squeezenet1_1; every other id in [7000, 8000) is MPX_E_ARG (squeezenet1_0 -- a 7x7 stride-2 unpadded stem and a
 *                                 ceil-mode pool whose last window hangs over the edge -- included)
 * A SqueezeNet engine runs features.0 (3 -> 64, 3x3 stride 2 WITHOUT padding, 224 -> 111, reading the padded NHWC4 staging: k_packed = 96) +
 * ReLU, eight Fire modules features.N = Fire(cin, s, e, e), (N, cin, s, e) = (3,64,16,64) (4,128,16,64) (6,128,32,128) (7,256,32,128)
 * (9,256,48,192) (10,384,48,192) (11,384,64,256) (12,512,64,256) -- squeeze 1x1 + ReLU, then expand1x1 and expand3x3 (pad 1) on the squeeze map,
 * each + ReLU, concatenated along the channels --, the max pools features.2 / .5 / .8 in front of Fire 3, 6 and 9 (MaxPool2d(3, 2,
 * ceil_mode=True) on 111 -> 55 -> 27 -> 13: hin - 3 is even in all three, so ceil mode equals floor mode, every window lies inside the map and
 * mpx_maxpool3x3s2p0 serves them), classifier.1 (512 -> 1000, 1x1) + ReLU on the 13x13 map and mpx_global_avgpool_logits.  Every conv has a
 * bias and there is no BatchNorm (bn_name ""; the bias loads as `beta`, as on the plain VGGs).  26 entries in the conv list.
 * THE CONCATENATION IS THE EXPAND CONVS' EPILOGUE.  expand1x1 writes channels [0, e) and expand3x3 channels [e, 2e) of the same planes
 * [B][h][h][2e] (mpx_conv_out_slice: row pitch 2e, channel offset 0 or e); nothing joins or copies them.  Such OUTPUT-SLICE layers run the
 * generic tiles 0, 1, 2, 4 and 7 only, take no residual operand, and mpx_conv_bn_act on one of them takes the BASE of the concatenated planes.
 * THE LAST CONV ENTRY IS NOT THE LOGIT LAYER HERE.  classifier.1 is followed by ReLU and the average pool, so in mpx_conv_bn_act it behaves
 * like any other layer: split planes [B][13][13][1000] out, out_f32 must be NULL; the logits are mpx_global_avgpool_logits' output.
 * Squeeze widths 16 and 48 are stored with a pitch of 32 and 64 (zero weight columns, zero scale and shift on the padded rows: exact zeros).
 * Three activation buffers of 111 * 111 * 64 elements per image (a module's input, its squeeze map, the concatenation): 10.3 MB per slot with
 * the staging.  It stages through mpx_mask_apply_normalize only: the stem-table and stem + pool entry points return MPX_E_STATE.
 * -- or torchvision's GoogLeNet (aux_logits off, eval mode; 6.6 M parameters, 1.5 GMAC per forward):
 *   MPX_ARCH_GOOGLENET            googlenet; every other id in [8000, 9000) is MPX_E_ARG
 * A GoogLeNet engine runs conv1 (3 -> 64, 7x7 stride 2 pad 3, 224 -> 112: the ResNet stem's shape, as a launch of its own), maxpool1, conv2
 * (1x1 64 -> 64), conv3 (3x3 pad 1 64 -> 192), maxpool2, inception3a / 3b, maxpool3, inception4a .. 4e, maxpool4 (2x2 stride 2, exact:
 * mpx_maxpool2x2s2), inception5a / 5b, mpx_global_avgpool and fc 1024 -> 1000, the logit layer and last conv entry as on a ResNet.  Every
 * conv is BasicConv2d = Conv2d(bias=False) + BatchNorm2d(eps = 0.001) + ReLU: names "<module>.conv", bn names "<module>.bn" ("conv1.conv",
 * "inception3a.branch2.1.conv"); the caller passes eps = 1e-3.  58 entries in the conv list: conv1, conv2, conv3, six per Inception module
 * (branch1, branch2.0, branch2.1, branch3.0, branch3.1, branch4.1), fc.
 * THE POOLS.  maxpool1 / 2 / 3 are MaxPool2d(3, 2, ceil_mode=True) on 112 -> 56 -> 28 -> 14: hin - 3 is odd, the last window hangs over the
 * edge; every Inception module's branch4 starts with MaxPool2d(3, 1, 1, ceil_mode=True).  All twelve run mpx_maxpool3x3_clip.
 * THE CONCATENATION IS THE BRANCHES' EPILOGUE, as SqueezeNet's: branch1, branch2.1, branch3.1 and branch4.1 write channels [0, c1), [c1, c1 +
 * c3), [c1 + c3, c1 + c3 + c5) and [c1 + c3 + c5, out) of one buffer (mpx_conv_out_slice); such OUTPUT-SLICE layers run the generic tiles
 * 0, 1, 2, 4 and 7 only and take no residual operand.
 * Reduce widths 16, 24, 48, 112 and 144 are stored with a pitch of 32, 32, 64, 128 and 160 (exact zeros in the padded channels).
 * inception4d's 528-channel concatenation is stored with a pitch of 544 and its branch4.1 (64 channels at offset 464) stores 80 channels, so
 * channels 528 .. 543 are written as exact zeros by every forward; inception4e's 1x1 convs and its pool read that pitch.
 * Three activation buffers of 112 * 112 * 64 elements per image (the stem's output): 10.5 MB per slot with the staging.  It stages through
 * mpx_mask_apply_normalize only: the stem-table and stem + pool entry points return MPX_E_STATE.  torchvision's transform_input (on in its
 * pretrained googlenet) is NOT applied: the caller's normalisation is the network's input.
 * -- or one of torchvision's ShuffleNetV2 networks (1.4 .. 7.4 M parameters, 0.04 .. 0.58 GMAC per forward):
 *   MPX_ARCH_SHUFFLENET + 5 / 10 / 15 / 20   shufflenet_v2_x0_5 / x1_0 / x1_5 / x2_0; every other id in [9000, 10000) is MPX_E_ARG
 * A ShuffleNetV2 engine runs conv1 (3 -> 24, 3x3 stride 2 pad 1, reading the padded NHWC4 staging: k_packed = 96) + BN + ReLU, the padded
 * 3x3 stride-2 max pool (mpx_maxpool3x3s2, 112 -> 56), stage2 / stage3 / stage4 of 4 / 8 / 4 blocks on 28x28 / 14x14 / 7x7 maps, conv5 (1x1 to
 * 1024, 2048 for x2_0) + BN + ReLU, mpx_global_avgpool and fc, the logit layer and last conv entry.  Stage widths (stage2, stage3, stage4):
 * x0_5 48, 96, 192; x1_0 116, 232, 464; x1_5 176, 352, 704; x2_0 244, 488, 976.  With bf = half a stage's width, a block is
 *   stride 1: x1, x2 = the halves of its input; cat(x1, branch2(x2));   stride 2 (block 0 of a stage): cat(branch1(x), branch2(x))
 *   branch2 = 1x1 conv + BN + ReLU, depthwise 3x3 + BN WITHOUT activation, 1x1 conv + BN + ReLU;  branch1 = depthwise 3x3 stride 2 + BN, 1x1 conv + BN + ReLU
 * followed by channel_shuffle(., 2).  38 entries in the conv list ("conv1.0", "stage2.0.branch1.2", "stage2.0.branch2.0", "stage2.0.branch2.5",
 * "stage2.1.branch2.0", ..., "conv5.0", "fc"; bn names "conv1.1", "stageN.k.branch1.3", ...), 19 depthwise layers in the depthwise list
 * ("stageN.0.branch1.0", "stageN.k.branch2.3"; clamp_in 0, linear: mpx_dwconv_layout, mpx_dwconv3x3_bn), 16 shuffles (mpx_num_shuffles).
 * THE TWO-HALF LAYOUT.  A stage map of 2 bf logical channels is stored with pitch 2 hp, hp = bf rounded up to 32: logical channel l < bf at
 * physical l, l >= bf at hp + (l - bf); physical channels [bf, hp) and [hp + bf, 2 hp) are exact zeros that every forward writes.  (bf, hp) of
 * stage2 / 3 / 4: x0_5 (24, 32) (48, 64) (96, 96); x1_0 (58, 64) (116, 128) (232, 256); x1_5 (88, 96) (176, 192) (352, 352); x2_0 (122, 128)
 * (244, 256) (488, 512).  A stride-1 block's branch2.0 is an INPUT-SLICE layer: it reads the second half in place (mpx_conv_in_slice: pitch
 * 2 hp, offset hp, K = hp), and mpx_conv_bn_act on it takes the BASE of the stage planes, as an output-slice layer takes the base of the
 * concatenation.  A stride-2 block's branch1.2 and branch2.5 are output-slice layers: they write the halves of one buffer (pitch 2 hp, offset
 * 0 / hp, hp channels stored: the pads as zeros).  mpx_shuffle2_concat interleaves the halves into the next two-half map.  A layer that reads
 * a whole stage map -- the next stage's branch1.0, branch1.2 and branch2.0, and conv5 -- has its weights placed at the physical channels
 * (mpx_conv_in_slice / mpx_dwconv_layout report bf and hp; mpx_pack_conv_weights, which sees the descriptor alone, packs the dense layout).
 * Input-slice, output-slice and padded layers run the generic tiles 0, 1, 2, 4 and 7 only.  conv1 and the pool keep 24 channels at pitch 32.
 * Three activation buffers of 112 * 112 * 32 elements per image (conv1's output) for every width: 5.7 MB per slot with the staging.  It
 * stages through mpx_mask_apply_normalize only: the stem-table and stem + pool entry points return MPX_E_STATE.
 * -- or torchvision's EfficientNet-B0 (5.3 M parameters, 0.39 GMAC per forward), the one EfficientNet whose native resolution is 224 x 224:
 *   MPX_ARCH_EFFICIENTNET + 0     efficientnet_b0; every other id in [10000, 11000) is MPX_E_ARG
 * An EfficientNet-B0 engine runs features.0 (3 -> 32, 3x3 stride 2 pad 1, reading the padded NHWC4 staging: k_packed = 96) + BN + SiLU, 16
 * MBConv blocks features.S.B over seven stages (expand ratio, kernel, stride, in, out, blocks) = (1,3,1,32,16,1) (6,3,2,16,24,2)
 * (6,5,2,24,40,2) (6,3,2,40,80,3) (6,5,1,80,112,3) (6,5,2,112,192,4) (6,3,1,192,320,1), features.8 (320 -> 1280, 1x1) + BN + SiLU,
 * mpx_global_avgpool_silu and classifier.1 (Linear(1280, 1000), the logit layer and last conv entry).  A block with input cin and expanded
 * width e = t * cin is 1x1 expand + BN + SiLU (absent when t = 1), depthwise k x k + BN + SiLU (mpx_dwconv_bn_act), SqueezeExcitation(e, q =
 * max(1, cin / 4)) (mpx_se_gate, then mpx_se_scale in place), 1x1 project + BN without activation, plus the block input when stride is 1 and
 * cin == out (the residual operand of the project conv; nothing behind the add).  34 entries in the conv list ("features.0.0",
 * "features.1.0.block.2.0", "features.2.0.block.0.0", "features.2.0.block.3.0", ..., "features.8.0", "classifier.1"), 16 depthwise layers
 * ("features.1.0.block.0.0", "features.2.0.block.1.0", ...; mpx_dwconv_shape reports kernel size and activations) and 16 SE layers
 * ("features.1.0.block.1", "features.2.0.block.2", ...; mpx_num_se / mpx_se_info / mpx_load_se).  mpx_forward launches the stem, per block
 * expand (absent in 1.0), depthwise, gate, scale, project, then features.8, the SiLU pool, classifier.1 and the head: 34 + 16 + 16 + 16 + 1 + 1.
 * THE SiLU BELONGS TO THE CONSUMER.  The MFMA conv kernels' epilogues know ReLU only, and SiLU cannot be had from ReLU by a clamp: a conv that
 * torchvision follows with SiLU (the stem, every expand conv, features.8) has relu = 0 in its descriptor and stores bn(conv(x)); its one
 * consumer takes silu(x) = x / (1 + expf(-x)) as it loads -- a depthwise layer (act_in = 1) or the SiLU global pool.  mpx_conv_bn_act on such
 * a layer therefore returns the PRE-ACTIVATION bn(conv(x)), not silu(.); mpx_conv_consumer_act says which layers these are and mpx_conv_desc
 * keeps its layout.  The depthwise kernel applies its own SiLU in its epilogue.
 * Channel counts 16, 24, 40, 80, 112, 144 and 240 are stored with a pitch of 32, 32, 64, 96, 128, 160 and 256 (exact zeros in the padded
 * channels, as MobileNetV2); such layers run the generic tiles only.
 * Three activation buffers of 112 * 112 * 96 elements per image (features.2.0's expanded map, MobileNetV2's size: 14.45 MB) plus the
 * staging (0.85 MB) and the SE gates (f32[1152], 4.6 KB): 15.3 MB per slot.  It stages through mpx_mask_apply_normalize only: the stem-table
 * and stem + pool entry points return MPX_E_STATE.
 * -- or one of torchvision's two 32-group ResNeXts, the members of the ResNet family whose Bottleneck has groups = 32 (25.0 M / 88.8 M parameters,
 * 4.2 / 16.4 GMAC per forward):
 *   MPX_ARCH_RESNEXT + 50 / 101   resnext50_32x4d / resnext101_32x8d; every other id in [11000, 12000) is MPX_E_ARG (resnext101_64x4d included)
 * A ResNeXt engine is the ResNet-50 / ResNet-101 engine -- the same stem and both stagings (mpx_mask_apply_normalize and the stem table), the
 * same layer names, block depths (3, 4, 6, 3) / (3, 4, 23, 3), block outputs 256, 512, 1024, 2048, conv3 + downsample launches
 * (mpx_conv_dual_bn_act), average pool and fc -- with an inner width of planes * width_per_group / 64 * 32 instead of planes: 128, 256, 512,
 * 1024 (32x4d) or 256, 512, 1024, 2048 (32x8d).  conv1 and conv3 are dense 1x1 layers of those widths.  conv2 is the GROUPED 3x3 conv, width ->
 * width in 32 groups of cg = width / 32 = 4, 8, 16, 32 (32x4d) or 8, 16, 32, 64 (32x8d) channels, stride 2 in the first block of layer2 / 3 /
 * 4: mpx_conv_groups reports 32 on it, its weight tensor is torchvision's [width][cg][3][3], and it runs the grouped kernel, tile 16
 * (csrc/mpx_gconv.h), through mpx_conv_bn_act like any other layer.  Its descriptor keeps mpx_conv_desc's layout with cin = cout = cout_pad =
 * width and k_packed = the K of ONE channel block of max(cg, 16) channels, 9 * max(cg, 16) rounded up to 32 (160, 288 or 576); mpx_pack_conv_weights,
 * which sees the descriptor alone, stays the dense packer and does not serve it.  No block tails and no pointwise tails (their shapes are
 * the ResNets').  Four activation buffers of 56 * 56 * 256 elements per image as on a ResNet (14.5 MB per slot with the staging and the
 * pooled stem planes) for 32x4d; of 56 * 56 * 512 (layer2.0.conv1's output) for 32x8d: 27.3 MB per slot.
 * -- or one of torchvision's two ConvNeXts of width 96, the first networks here with LayerNorm and GELU instead of BatchNorm and a ReLU-family
 * activation (28,589,128 / 50,223,688 parameters, 4,455,531,264 / 8,683,712,256 MAC per forward):
 *   MPX_ARCH_CONVNEXT + 1 / 2     convnext_tiny / convnext_small (depths (3, 3, 9, 3) / (3, 3, 27, 3), dims (96, 192, 384, 768)); every other id
 *                                 in [12000, 13000) is MPX_E_ARG (convnext_base / convnext_large -- dims from 128 / 192 -- included)
 * A ConvNeXt engine runs features.0.0 (3 -> 96, 4x4 stride 4 WITHOUT padding, bias, 224 -> 56, reading the padded NHWC4 staging 3 pixels into
 * its border: k_packed = 4 * 32 = 128 under the `ky*32 + px*4 + c` rule, zero weights on px >= 4) and features.0.1 = LayerNorm2d(96) as a launch
 * of its own (mpx_layernorm_c), then four stages features.1 / .3 / .5 / .7 of CNBlocks of width C = 96, 192, 384, 768 on 56 / 28 / 14 / 7 maps.
 * A CNBlock features.S.B is block.0 = depthwise 7x7 (pad 3, bias) and block.2 = LayerNorm(C) over the channels of each pixel in ONE launch
 * (mpx_dwconv7x7_ln), block.3 = Linear(C, 4C) + GELU and block.5 = Linear(4C, C) as 1x1 entries of the conv list, and output = input +
 * layer_scale * block(input) with nothing behind the add.  features.2 / .4 / .6 are LayerNorm2d(C_prev) (.0: mpx_layernorm_c) and Conv2d(C_prev,
 * C, 2, stride 2, bias) (.1: an ordinary 2x2 entry of the conv list, k_packed = 4 * C_prev); the head is the global average pool with
 * classifier.0 = LayerNorm2d(768) behind it in one launch (mpx_global_avgpool_ln) and classifier.2 = Linear(768, 1000), the logit layer and
 * last conv entry.  Every LayerNorm has eps 1e-6.  41 / 77 entries in the conv list ("features.0.0", "features.1.0.block.3",
 * "features.1.0.block.5", ..., "features.2.1", ..., "classifier.2"), 18 / 36 depthwise layers ("features.1.0.block.0", ...; bn_name is the
 * LayerNorm's prefix "features.1.0.block.2"; mpx_dwconv_shape reports ksize 7, mpx_dwconv_ln the fused LayerNorm; mpx_load_dwconv_ln loads
 * them), 5 stand-alone LayerNorms (mpx_num_lnorms: "features.0.1", "features.2.0", "features.4.0", "features.6.0", "classifier.0").
 * mpx_forward launches the stem conv, its LayerNorm, per block depthwise + LayerNorm, block.3, block.5, per stage boundary the LayerNorm and
 * the 2x2 conv, then the pooled LayerNorm, classifier.2 and the head: 2 + 3 * 18 + 2 * 3 + 3 = 65 launches (tiny), 2 + 3 * 36 + 6 + 3 = 119 (small).
 * GELU IS IN THE EPILOGUE.  block.3's consumer is another MFMA conv, so its activation cannot ride on a consumer's load: the generic kernel's
 * epilogue has the exact GELU as a compile-time constant of the tile class (csrc/mpx_conv.h, ConvGelu).  mpx_conv_epilogue_act reports 1 on
 * such a layer, relu is 0 in its descriptor and mpx_conv_consumer_act stays 0; mpx_conv_bn_act returns gelu(W x + b).  Such a layer runs the
 * generic tiles 0, 1, 2, 4 and 7 only (default 7).
 * LAYER SCALE IS THE SCALE OF block.5's EPILOGUE.  block.5 is an ordinary entry with residual = 1, relu = 0 whose bn_name is the block's
 * "features.S.B.layer_scale": the caller passes conv_bias = block.5.bias, gamma = layer_scale, beta = 0, mean = 0, var = 1 and eps = 0, which
 * the packer turns into scale = layer_scale * 2^-e, shift = bias * layer_scale exactly.
 * Every channel count (96 .. 3072) is a multiple of 32: no padded pitches.  Three activation buffers of 56 * 56 * 384 elements per image
 * (block.3's output in stage 0, 1.5 x a ResNet buffer, MobileNetV2's size: 14.45 MB) -- X the block input and residual, T1 the LayerNorm
 * output and then, dead after block.3, the block output, T2 the hidden map -- plus the staging (0.85 MB): 15.3 MB per slot.  It stages through
 * mpx_mask_apply_normalize only: the stem-table and stem + pool entry points return MPX_E_STATE.
 * -- or one of torchvision's two ViT-Base networks, the first here that are no CNN (86,567,656 / 88,224,232 parameters, 17,563,828,224 /
 * 4,409,186,304 MAC per forward, the attention products Q K^T and P V counted: 2 * T^2 * 64 * 12 per layer):
 *   MPX_ARCH_VIT + 16 / 32        vit_b_16 / vit_b_32 (patch 16 / 32, T = 197 / 50 tokens, 12 layers of width D = 768, 12 heads of 64, MLP 3072);
 *                                 every other id in [13000, 14000) is MPX_E_ARG (vit_l_16 / vit_l_32 / vit_h_14 and the Swin family are not served)
 * A ViT engine runs conv_proj (3 -> 768, p x p stride p WITHOUT padding, bias, reading the padded NHWC4 staging 3 pixels into its border: one
 * p-pixel x 4-channel run per kernel row, k_packed = p * 4p = 16 * 64 / 32 * 128, zero weights on channel 3) into planes [B][T - 1][768], the token
 * assembly (mpx_tokens_assemble: class_token and encoder.pos_embedding, mpx_load_tokens), then 12 encoder layers of 7 launches each -- ln_1
 * (mpx_layernorm_c on the B * T rows), self_attention.in_proj (768 -> 2304, bias), the attention (mpx_attention), self_attention.out_proj
 * (768 -> 768, bias, residual), ln_2, mlp.0 (768 -> 3072, GELU in the epilogue as a ConvNeXt block.3: mpx_conv_epilogue_act) and mlp.3 (3072 ->
 * 768, bias, residual) --, encoder.ln on the class-token row of each image alone (mpx_layernorm_rows, rows T apart -> planes [B][768]),
 * heads.head (the logit layer and last conv entry) and the head: 2 + 7 * 12 + 3 = 89 launches.  Every LayerNorm has eps 1e-6.
 * TOKEN LAYERS ARE NO SQUARE MAPS (197 is prime): the Linear layers of the encoder are 1x1 entries of the conv list that report hin = hout = 0;
 * mpx_conv_rows reports their T rows per image (0 on every layer of every other engine), and their planes are [B][T][cin] -> [B][T][cout].
 * DESCRIPTOR NAMES DROP THE LEADING "encoder.layers." (name[48] cannot hold "encoder.layers.encoder_layer_11.self_attention.out_proj"):
 * "encoder_layer_11.self_attention.out_proj", "encoder_layer_0.ln_1", "encoder_layer_3.self_attention"; a loader puts the prefix back on every
 * name that starts with "encoder_layer_".  in_proj's tensors are `<prefix>.self_attention.in_proj_weight` / `in_proj_bias` in torchvision's
 * state_dict (an underscore, nn.MultiheadAttention's parameters), every other layer's `<name>.weight` / `<name>.bias`.
 * A bias-only layer has no bn_name; mpx_set_conv_weights takes its bias as conv_bias with gamma = 1, beta = 0, mean = 0, var = 1, eps = 0, which
 * packs to scale = 2^-e, shift = bias exactly -- there is no second epilogue form.  50 entries in the conv list ("conv_proj",
 * "encoder_layer_0.self_attention.in_proj", "....out_proj", "encoder_layer_0.mlp.0", "encoder_layer_0.mlp.3", ..., "heads.head"), 25 stand-alone
 * LayerNorms ("encoder_layer_0.ln_1", "encoder_layer_0.ln_2", ..., "encoder.ln"; hw = 0), 12 attention launches (mpx_num_attn).
 * Four activation buffers per image, each of its own size: X (T * 768, the residual stream), T1 (T * 768: the patch planes, a LayerNorm's
 * output, the attention's), QKV (T * 2304: in_proj's output and then, dead behind the attention, out_proj's) and H (T * 3072): 5.45 MB / 1.38 MB
 * plus the staging (0.85 MB): 6.3 / 2.2 MB per slot.  It stages through mpx_mask_apply_normalize only: the stem-table and stem + pool entry
 * points return MPX_E_STATE.
 * -- or one of torchvision's five RegNetX networks up to 8 GF, whose bottleneck's 3x3 is grouped by a fixed GROUP WIDTH, so that the group count
 * is whatever the stage width gives (5,495,976 / 7,259,656 / 9,190,136 / 15,296,552 / 39,572,648 parameters, 413,812,608 / 799,699,712 /
 * 1,602,849,792 / 3,176,621,952 / 7,995,132,416 MAC per forward):
 *   MPX_ARCH_REGNET + 4 / 8 / 16 / 32 / 80   regnet_x_400mf / _800mf / _1_6gf / _3_2gf / _8gf (ten times the GF figure); every other id in
 *                                            [14000, 15000) is MPX_E_ARG (regnet_x_16gf / _32gf included)
 *   stage widths (32, 64, 160, 400) (64, 128, 288, 672) (72, 168, 408, 912) (96, 192, 432, 1008) (80, 240, 720, 1920), depths (1, 2, 7, 12)
 *   (1, 3, 7, 5) (2, 4, 10, 2) (2, 6, 15, 2) (2, 5, 15, 1), group width 16, 16, 24, 48, 120 -- groups (2, 4, 10, 25) (4, 8, 18, 42) (3, 7, 17, 38)
 *   (2, 4, 9, 21) (1, 2, 6, 16); 72 / 54 / 60 / 81 / 75 entries in the conv list.
 * A RegNetX engine runs stem.0 (3 -> 32, 3x3 stride 2 pad 1, BatchNorm stem.1, ReLU: MobileNetV2's features.0.0 shape, k_packed = 96, no max
 * pool) and four stages trunk_output.block{s}.block{s}-{j} of bottlenecks of ratio 1: f.a.0 (1x1 w_in -> w, BN f.a.1, ReLU, at the input
 * resolution), f.b.0 (3x3 w -> w pad 1 in w / gw groups, stride 2 in block 0 of EVERY stage, BN f.b.1, ReLU), f.c.0 (1x1 w -> w, BN f.c.1,
 * residual = 1: ReLU(shortcut + f.c)), with proj.0 (1x1 stride 2, BN proj.1, no activation) as the shortcut in block 0 -- a launch of its
 * own, listed in front of f.a.0 as in torchvision's state_dict -- and the identity elsewhere; then the global average pool, fc and the head.
 * f.b IS THE GROUPED LAYER: mpx_conv_groups reports w / gw on it (1 on the dense 80 -> 80 3x3 of regnet_x_8gf's first stage, an ordinary
 * entry on the ordinary kernels), its weight tensor is torchvision's [w][gw][3][3], and it runs tile 18 (csrc/mpx_gconvw.h).  Its descriptor
 * has cin = cout = w, k_packed = 9 * gw rounded up to 32 (160, 224, 448, 1088) and cout_pad = groups * ceil(gw / 16) * 16, the rows of its packed
 * planes; mpx_pack_conv_weights does not serve it.
 * Widths that are no multiple of 32 (72, 80, 168, 240, 400, 408, 432, 720, 912, 1008) are stored with a pitch of the next multiple of 32
 * (exact zeros in the padded channels, as MobileNetV2: the grouped kernel writes them itself); such dense layers run the generic tiles only.
 * Four activation buffers of the network's largest map (112 * 112 * 32 / 64 / 96 / 96 / 96 elements per image) plus the staging.  It stages
 * through mpx_mask_apply_normalize only: the stem-table and stem + pool entry points return MPX_E_STATE.
 * -- or one of torchvision's RegNetY networks from 800 MF to 8 GF: RegNetX's trunk with a Squeeze-and-Excitation gate in every block
 * (6,432,512 / 11,202,430 / 19,436,338 / 39,381,472 parameters):
 *   MPX_ARCH_REGNET_Y + 8 / 16 / 32 / 80     regnet_y_800mf / _1_6gf / _3_2gf / _8gf (ten times the GF figure); every other id in
 *                                            [15000, 16000) is MPX_E_ARG (regnet_y_400mf: a group width of 8, below the grouped kernel's 16;
 *                                            regnet_y_16gf / _32gf: group widths 112 / 232 = 7 / 15 row fragments, no whole number of chunks)
 *   stage widths (64, 144, 320, 784) (48, 120, 336, 888) (72, 216, 576, 1512) (224, 448, 896, 2016), depths (1, 3, 8, 2) (2, 6, 17, 2)
 *   (2, 5, 13, 1) (2, 4, 10, 1), group width 16, 24, 24, 56 -- groups (4, 9, 20, 49) (2, 5, 14, 37) (3, 9, 24, 63) (4, 8, 16, 36); 48 / 87 / 69 /
 *   57 entries in the conv list, 14 / 27 / 21 / 17 in the SE list.
 * Stem, blocks, pitches, buffers and staging are RegNetX's.  The one addition: between f.b and f.c every block has f.se =
 * SqueezeExcitation(w, q) with q = the BLOCK's input width / 4 (32 / 4 = 8 in block1-0, the previous stage's width / 4 in the other stage
 * openers), fc1 and fc2 1x1 convs WITH bias, ReLU behind fc1 and sigmoid behind fc2: mpx_forward runs mpx_se_gate_relu and mpx_se_scale in
 * place on f.b's output (mpx_num_se, mpx_se_info, mpx_load_se, mpx_se_params, mpx_se_act = 1; state_dict keys <block>.f.se.fc1.weight / .bias,
 * .fc2.weight / .bias).  regnet_y_8gf's group width 56 is tile 18's fifth instantiation (4 row fragments, K = 504 padded to 512).
 * Small-network engines stage inputs with mpx_mask_apply_minmax (their scorers' mask convention) instead of
 * mpx_mask_apply_normalize, keep activations as NHWC planes with channels padded to a multiple of 32, and score 10 classes
 * (logit rows are 16 floats apart: mpx_geometry). */
#define MPX_ARCH_MNIST_NET 1
#define MPX_ARCH_CIFAR_RESNET 2000
#define MPX_ARCH_VGG 3000
#define MPX_ARCH_VGG_BN 3100
#define MPX_ARCH_ALEXNET 4000
#define MPX_ARCH_DENSENET 5000
#define MPX_ARCH_MOBILENET 6000
#define MPX_ARCH_SQUEEZENET 7000
#define MPX_ARCH_GOOGLENET 8000
#define MPX_ARCH_SHUFFLENET 9000
#define MPX_ARCH_EFFICIENTNET 10000
#define MPX_ARCH_RESNEXT 11000
#define MPX_ARCH_CONVNEXT 12000
#define MPX_ARCH_VIT 13000
#define MPX_ARCH_REGNET 14000
#define MPX_ARCH_REGNET_Y 15000
typedef struct mpx_engine mpx_engine;

typedef struct mpx_conv_desc {
    char name[48];       /* torchvision state_dict prefix of the conv ("layer3.4.conv2", "fc", "features.7", "classifier.0") */
    char bn_name[48];    /* prefix of its BatchNorm ("layer3.4.bn2", "features.8"); "" for a layer without one (fc, plain VGG) */
    int32_t cin, cout, ksize, stride, pad;
    int32_t hin, hout;   /* square spatial sizes at 224x224 input */
    int32_t relu;        /* ReLU in the epilogue */
    int32_t residual;    /* adds the block identity before the ReLU */
    int32_t k_packed;    /* K of the packed [cout_pad][k_packed] fp16 weight planes */
    int32_t cout_pad;    /* rows of the packed planes (multiple of 128) */
} mpx_conv_desc;

/* ---- engine life cycle -------------------------------------------------------------------
 * replaces: models.__dict__[args.arch](pretrained=True); model.cuda(); model.eval()
 *           (generate_gp_training_data_imagenet.py:579-580,159).  Allocates the whole workspace
 *           (input staging for max_batch masked images, activation planes, logits) once. */
int mpx_create(int arch_id, int max_batch, int device, mpx_engine** out);
int mpx_destroy(mpx_engine* h);
const char* mpx_last_error(const mpx_engine* h);   /* "" if none; valid until next call */
int mpx_max_batch(const mpx_engine* h);
/* Compute units of the engine's device (hipDeviceAttributeMultiprocessorCount, read by mpx_create): the persistent kernels launch
 * one workgroup per CU, so a forward batch is best a whole number of `num_cus * 256`-pixel rounds of the 14x14 maps
 * (engine.whole_round_batch). */
int mpx_num_cus(const mpx_engine* h);
/* 224/3/1000/1000 for the ImageNet ResNets and ResNeXts, the VGG networks, AlexNet, the DenseNets, MobileNetV2, SqueezeNet 1.1, GoogLeNet, the ShuffleNetV2s and EfficientNet-B0, 28/1/10/16 and 32/3/10/16 for the small networks; any pointer may be NULL */
int mpx_geometry(const mpx_engine* h, int* image_size, int* in_channels, int* num_classes, int* logit_pitch);
size_t mpx_workspace_bytes(const mpx_engine* h);

/* ---- topology / weights ------------------------------------------------------------------
 * Layer i in [0, mpx_num_convs): every conv in forward order; the last entry is the logit layer, whatever its name ("fc", "fc1",
 * "classifier.6") -- except on a SqueezeNet engine, whose last entry (classifier.1) writes planes like any other layer and whose logits come
 * out of mpx_global_avgpool_logits. */
int mpx_num_convs(const mpx_engine* h);
int mpx_conv_info(const mpx_engine* h, int i, mpx_conv_desc* out);
/* The layer plan build_topology makes for arch_id, as text; no engine, no device, no HIP call.  One record per line, "<section> [<index>]
 * key=value ...": `engine` (the geometry and buffer plan), `conv` (every mpx_conv_desc field and the layer's layout, tile and fusion
 * fields), the four op lists `ops` / `ops_bt` / `ops_pt` / `ops_pt0`, then `tail`, `ptail`, `norm`, `dw`, `lnorm`, `attn`, `se`, `shuffle`,
 * `pool3c`.  Deterministic for an arch id; no pointer, no device property.
 * *len = bytes needed (without the NUL), always set; buf == NULL: only that.  cap <= *len: MPX_E_ARG, nothing written.
 * An arch id mpx_create rejects returns what mpx_create returns for it. */
int mpx_describe_plan(int arch_id, char* buf, size_t cap, size_t* len);
/* Where layer i writes: *pitch = channels between adjacent pixels of its output planes, *offset = its first channel within a pixel.  An
 * ordinary layer fills whole pixel rows: its stored channel count (cout, or cout rounded up to 32 where the network pads) and 0.  A
 * SqueezeNet expand conv writes half of its Fire module's concatenation: 2 * cout and 0 (expand1x1) or cout (expand3x3).  A GoogLeNet branch's
 * last conv writes its range of the Inception module's concatenation: the concatenation's width rounded up to 32 (544 for inception4d's 528)
 * and 0 (branch1), c1 (branch2.1), c1 + c3 (branch3.1) or c1 + c3 + c5 (branch4.1).  In general a slice is any pitch, offset and stored
 * width that are multiples of 8 with offset + stored width <= pitch; the stored width is cout, except where the last slice also writes the
 * concatenation's pad channels as zeros (inception4d.branch4.1: cout 64, 80 stored).  mpx_conv_desc keeps its layout. */
int mpx_conv_out_slice(const mpx_engine* h, int i, int* pitch, int* offset);
/* Where layer i reads: *pitch = channels between adjacent pixels of its input planes, *offset = its first channel within a pixel.  An
 * ordinary layer reads whole pixel rows: k_packed / ksize^2 and 0 (4 and 0 for a layer on the NHWC4 staging).  A stride-1 ShuffleNetV2
 * block's branch2.0 reads the second half of a two-half stage map in place: 2 hp and hp (its k_packed is hp).  *bf, *hp: non-zero when the
 * layer reads a WHOLE two-half stage map (cin = 2 bf logical channels at pitch 2 hp): its weight column of logical channel l sits at l
 * (l < bf) or hp + l - bf; 0, 0 for every other layer.  Any pointer may be NULL. */
int mpx_conv_in_slice(const mpx_engine* h, int i, int* pitch, int* offset, int* bf, int* hp);
/* Groups of layer i: 32 on the conv2 of a ResNeXt engine's blocks (cin / 32 input channels per output channel: mpx_set_conv_weights takes
 * [cout][cin / 32][3][3] there, and the layer runs tile 16 and nothing else), w / gw = 2 .. 63 on the f.b of a RegNetX / RegNetY engine's blocks
 * ([w][gw][3][3]; tile 18, and tile 16 where the shape is one of that kernel's), 1 on every other layer of every engine. */
int mpx_conv_groups(const mpx_engine* h, int i, int* groups);
/* The activation torchvision puts behind layer i that the layer itself does NOT apply because its one consumer takes it on load: *act = 0
 * none (every layer of every other network; ReLU6's clamp is reported by mpx_dwconv_desc.clamp_in), 1 SiLU (an EfficientNet-B0 engine's stem,
 * expand convs and features.8: mpx_conv_bn_act returns bn(conv(x)) there). */
int mpx_conv_consumer_act(const mpx_engine* h, int i, int* act);
/* The activation layer i DOES apply in its epilogue besides what mpx_conv_desc.relu says: *act = 0 none (every layer of every other network),
 * 1 exact GELU (a ConvNeXt engine's block.3 layers: mpx_conv_bn_act returns gelu(W x + b), the layer runs the generic tiles 0, 1, 2, 4 and 7
 * only, and mpx_set_conv_tile refuses every other tile on it).  mpx_conv_desc keeps its layout. */
int mpx_conv_epilogue_act(const mpx_engine* h, int i, int* act);
/* The rows per image of layer i where they are no square map: *rows_per_image = T on a ViT engine's token layers (in_proj, out_proj, mlp.0,
 * mlp.3: mpx_conv_desc reports hin = hout = 0 there and the planes are [B][T][channels]), 0 on every layer of every other engine and on a ViT
 * engine's conv_proj (a 14 x 14 / 7 x 7 map) and heads.head (one row per image). */
int mpx_conv_rows(const mpx_engine* h, int i, int* rows_per_image);

/* replaces: the state_dict tensors torchvision loads (same line as above).  HOST pointers, f32:
 * w = conv weight OIHW [cout][cin][k][k]; conv_bias = the conv's own bias [cout] or NULL (torchvision's ResNet convs have
 * none; the MNIST net's nn.Conv2d do, generate_gp_training_data_mnist.py:72-77); gamma/beta/mean/var = BatchNorm
 * weight/bias/running_mean/running_var [cout]; eps = 1e-5.  For a layer without BatchNorm (bn_name "": "fc", the MNIST
 * net's "conv6"): beta = its bias, gamma/mean/var/conv_bias = NULL.  Packs on the host (mpx_pack_conv_weights) and
 * uploads synchronously. */
int mpx_set_conv_weights(mpx_engine* h, int i, const float* w, const float* conv_bias, const float* gamma,
                         const float* beta, const float* mean, const float* var, float eps);
int mpx_weights_complete(const mpx_engine* h);     /* 1 when every layer has weights (and every stand-alone BatchNorm, depthwise and SE layer its vectors) */

/* ---- stand-alone BatchNorms (DenseNet) -------------------------------------------------------
 * Norm k in [0, mpx_num_norms): the BatchNorm2d modules that precede their conv, in forward order ("features.denseblock1.denselayer1.norm1",
 * ..., "features.transition1.norm", ..., "features.norm5"); 0 norms on every other architecture.  mpx_load_norm takes the HOST f32[channels]
 * tensors of torchvision's state_dict (<name>.weight / .bias / .running_mean / .running_var) and uploads, synchronously, the fp32 vectors
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale (computed in double, rounded once).  mpx_norm_params returns their DEV
 * pointers (f32[channels] each; what mpx_forward hands to mpx_concat_bn_relu). */
typedef struct mpx_norm_desc {
    char name[64];       /* torchvision state_dict prefix of the BatchNorm */
    int32_t channels;    /* C: the channels of the concatenation it normalises */
    int32_t hw;          /* side of the square map it runs on at 224x224 input */
} mpx_norm_desc;
int mpx_num_norms(const mpx_engine* h);
int mpx_norm_info(const mpx_engine* h, int k, mpx_norm_desc* out);
int mpx_load_norm(mpx_engine* h, int k, const float* gamma, const float* beta, const float* mean, const float* var, float eps);
int mpx_norm_params(const mpx_engine* h, int k, const float** scale, const float** shift);

/* ---- depthwise layers (MobileNetV2) ------------------------------------------------------------
 * Depthwise layer k in [0, mpx_num_dwconvs): the 3x3 depthwise convs in forward order ("features.1.conv.0.0", "features.2.conv.1.0", ...);
 * 0 on every other architecture.  mpx_load_dwconv takes the HOST f32 tensors of torchvision's state_dict -- w = <name>.weight
 * [channels][1][3][3] ([channels][1][5][5] on a 5x5 layer: mpx_dwconv_shape), gamma / beta / mean / var = <bn_name>.weight / .bias / .running_mean / .running_var [channels] -- and uploads,
 * synchronously, the fp32 tap-major weights [ksize^2][pitch] (tap = ky * ksize + kx; ksize = 3, or 5: mpx_dwconv_shape) and the vectors scale = gamma / sqrt(var + eps), shift = beta -
 * mean * scale [pitch] (computed in double, rounded once, as mpx_load_norm), zeros on channels [channels, pitch).  mpx_dwconv_params returns
 * their DEV pointers (what mpx_forward hands to the kernel).  mpx_weights_complete and mpx_forward count the depthwise layers. */
typedef struct mpx_dwconv_desc {
    char name[48];       /* torchvision state_dict prefix of the depthwise conv */
    char bn_name[48];    /* prefix of its BatchNorm */
    int32_t channels;    /* C: groups = in channels = out channels */
    int32_t pitch;       /* channels per pixel of its input and output planes (C rounded up to a multiple of 32) */
    int32_t stride;      /* 1 or 2; pad is 1, so hout = (hin - 1) / stride + 1 */
    int32_t hin;         /* side of the square input map at 224x224 input */
    int32_t clamp_in;    /* 1: the input is the ReLU output of an MFMA conv that torchvision follows with ReLU6; min(x, 6) is taken on load */
} mpx_dwconv_desc;
int mpx_num_dwconvs(const mpx_engine* h);
int mpx_dwconv_info(const mpx_engine* h, int k, mpx_dwconv_desc* out);
int mpx_load_dwconv(mpx_engine* h, int k, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps);
int mpx_dwconv_params(const mpx_engine* h, int k, const float** w, const float** scale, const float** shift);
/* What mpx_dwconv_desc has no field for (its layout is fixed): *linear = 1 when the layer has NO activation behind its BatchNorm and no clamp
 * on load (every depthwise layer of a ShuffleNetV2 engine: mpx_forward runs mpx_dwconv3x3_bn on it), 0 for MobileNetV2's ReLU6 layers; *bf,
 * *hp non-zero when its planes are a whole two-half stage map (channels = 2 bf at pitch 2 hp: channel c >= bf loads to hp + c - bf).  Any
 * pointer may be NULL. */
int mpx_dwconv_layout(const mpx_engine* h, int k, int* linear, int* bf, int* hp);
/* More of what mpx_dwconv_desc has no field for: *ksize = 3 or 5 (5 on an EfficientNet-B0 engine's stages 3, 5 and 6: mpx_load_dwconv takes
 * [channels][1][5][5] weights there and uploads [25][pitch], tap = ky * 5 + kx; pad is (ksize - 1) / 2), *act_in / *act_out = 1 where the
 * layer takes SiLU on load / applies SiLU behind its BatchNorm (every depthwise layer of an EfficientNet-B0 engine, whose clamp_in is 0:
 * mpx_forward runs mpx_dwconv_bn_act on it), 0 / 0 on every other engine.  Any pointer may be NULL. */
int mpx_dwconv_shape(const mpx_engine* h, int k, int* ksize, int* act_in, int* act_out);
/* Still more of what mpx_dwconv_desc has no field for: *ln = 1 when the layer is a ConvNeXt block's depthwise 7x7 conv WITH BIAS and the
 * LayerNorm over the channels fused behind it (mpx_dwconv_shape reports ksize 7 there; mpx_dwconv_desc.bn_name is the LayerNorm's prefix
 * "features.S.B.block.2"; mpx_forward runs mpx_dwconv7x7_ln on it), 0 on every other engine; *bias = the DEV f32[channels] conv bias (NULL
 * when *ln is 0), *eps = the LayerNorm's epsilon as loaded.  On such a layer mpx_dwconv_params returns w = the tap-major weights [49][channels],
 * scale = the LayerNorm's weight (gamma) and shift = its bias (beta).  Any pointer may be NULL.
 * mpx_load_dwconv's signature has no room for the conv bias, so a layer with *ln = 1 loads through mpx_load_dwconv_ln: HOST f32 w =
 * <name>.weight [channels][1][7][7], conv_bias = <name>.bias, ln_weight / ln_bias = <bn_name>.weight / .bias [channels], eps = 1e-6.
 * mpx_load_dwconv on such a layer, and mpx_load_dwconv_ln on any other, return MPX_E_ARG. */
int mpx_dwconv_ln(const mpx_engine* h, int k, int* ln, const float** bias, float* eps);
int mpx_load_dwconv_ln(mpx_engine* h, int k, const float* w, const float* conv_bias, const float* ln_weight, const float* ln_bias, float eps);

/* ---- stand-alone LayerNorms (ConvNeXt) ---------------------------------------------------------
 * LayerNorm k in [0, mpx_num_lnorms): the LayerNorm2d modules that are launches of their own, in forward order -- "features.0.1" (behind the
 * stem), "features.2.0" / "features.4.0" / "features.6.0" (in front of the 2x2 stride-2 convs; mpx_layernorm_c) and "classifier.0" (fused
 * behind the global average pool: mpx_global_avgpool_ln; hw = 1); 0 on every other architecture.  mpx_load_lnorm takes the HOST
 * f32[channels] tensors <name>.weight / <name>.bias and the module's eps (1e-6) and uploads them, synchronously, as they are.
 * mpx_lnorm_params returns their DEV pointers and the epsilon.  mpx_weights_complete and mpx_forward count them. */
typedef struct mpx_lnorm_desc {
    char name[64];       /* torchvision state_dict prefix of the LayerNorm2d */
    int32_t channels;    /* C: the channels of a pixel it normalises over */
    int32_t hw;          /* side of the square map it runs on at 224x224 input (1 for classifier.0, which runs on the pooled row) */
} mpx_lnorm_desc;
int mpx_num_lnorms(const mpx_engine* h);
int mpx_lnorm_info(const mpx_engine* h, int k, mpx_lnorm_desc* out);
int mpx_load_lnorm(mpx_engine* h, int k, const float* weight, const float* bias, float eps);
int mpx_lnorm_params(const mpx_engine* h, int k, const float** weight, const float** bias, float* eps);

/* ---- Squeeze-and-Excitation layers (EfficientNet-B0) --------------------------------------------
 * SE layer k in [0, mpx_num_se): the SqueezeExcitation modules in forward order ("features.1.0.block.1", "features.2.0.block.2", ...); 0 on
 * every other architecture.  mpx_load_se takes the HOST f32 tensors of torchvision's state_dict -- w1 = <name>.fc1.weight [q][channels][1][1],
 * b1 = <name>.fc1.bias [q], w2 = <name>.fc2.weight [channels][q][1][1], b2 = <name>.fc2.bias [channels] -- and uploads, synchronously, the
 * operands of mpx_se_gate: w1 as [q][pitch] with zero columns on channels [channels, pitch), w2 TRANSPOSED to [q][pitch] (w2[j][c] =
 * fc2.weight[c][j]) with zeros on the pads, b1 [q], b2 [pitch] with -inf on the pads (their gates come out as exact zeros).  mpx_se_params
 * returns their DEV pointers (what mpx_forward hands to the kernel).  mpx_weights_complete and mpx_forward count the SE layers. */
typedef struct mpx_se_desc {
    char name[48];       /* torchvision state_dict prefix of the SqueezeExcitation module ("features.3.1.block.2") */
    int32_t channels;    /* e: the expanded width it gates */
    int32_t pitch;       /* channels per pixel of the planes it reads and scales (e rounded up to a multiple of 32) */
    int32_t q;           /* squeeze width: max(1, block input channels / 4) */
    int32_t hw;          /* side of the square map it pools and scales at 224x224 input */
} mpx_se_desc;
int mpx_num_se(const mpx_engine* h);
int mpx_se_info(const mpx_engine* h, int k, mpx_se_desc* out);
int mpx_load_se(mpx_engine* h, int k, const float* w1, const float* b1, const float* w2, const float* b2);
int mpx_se_params(const mpx_engine* h, int k, const float** w1, const float** b1, const float** w2, const float** b2);
/* The activation behind fc1 of SE layer k: *act = 0 SiLU (every layer of an EfficientNet-B0 engine: mpx_forward runs mpx_se_gate), 1 ReLU
 * (every f.se of a RegNetY engine, q = block input width / 4: mpx_se_gate_relu).  MPX_E_ARG for a null pointer or a bad index. */
int mpx_se_act(const mpx_engine* h, int k, int* act);

/* Kernel variant of layer i (tuning / test hook; results are identical up to fp32 summation order).  The ids are exactly the
 * kernels some layer class runs by default:
 *   0 = 128x256 tile, 8 waves, 3-stage LDS ring, 1 workgroup per CU (wide stride-2 3x3 layers);
 *   1 = 64x256, 4 waves side by side (cout <= 64: the stem and the 64 -> 64 3x3 layers);
 *   2 = 128x128, 4 waves, 2-deep rings, 64 KB, 2 workgroups per CU (strided 1x1 layers, fc, everything without a better fit);
 *   4 = 64x192, 64 KB, 2 workgroups per CU (1x1 layers with cout = 64);
 *   6 = the 3x3 patch kernel (stride-1 3x3 layers whose input patch fits the LDS: the input is staged once per 32-channel chunk
 *       and the 9 taps read it at row offsets);
 *   7 = the 128x128 tile cut into 8 waves of 32x64 (124 VGPRs: two workgroups = 16 waves per CU; expanding 1x1 layers with
 *       K = 64 or on 7x7 maps, and the K-concatenated conv3 + downsample launches);
 *   9 = 256x256 tile, two 64-KB stages (reducing 1x1 stride-1 layers with cout % 256 == 0, cin % 64 == 0);
 *  10 = persistent pipelined 256x128 kernel, three stages running on across tiles (expanding 1x1 stride-1 layers with
 *       cout % 256 == 0, cin >= 128 that tile 14 does not take: 128 -> 512, 512 -> 2048);
 *  14 = the expanding 1x1 kernel whose weights live in registers (csrc/mpx_convw.h): one persistent 4-wave workgroup per CU on
 *       256 x 64 tiles, every wave keeps the 64 x 256 x (hi + lo) weights of its channels in 256 AGPRs, the LDS holds only two
 *       whole pixel tiles (1x1 stride-1 layers with cout % 256 == 0 and cin = 256: the default of 256 -> 1024 on 14x14 maps;
 *       bit-identical to 7 and 10);
 *  13 = the 256x256 kernel (9) as ONE persistent workgroup per CU: the two-stage ring runs on across tiles, register epilogue (layers
 *       eligible for 9 without a residual operand: their default; bit-identical to 9).  Its DUAL form runs the conv3 + downsample launch
 *       of a Bottleneck stage (mpx_conv_dual_bn_act) whose main layer sits on tile 9, 10, 13 or 14 -- 1x1 stride 1, cout % 256 == 0, both
 *       K segments multiples of 64 -- from one round of tiles on, and reports bit 13; under one round, and with the main layer on any other
 *       tile (7 and 2 force their own dual kernels), tile 7's or tile 2's dual kernel runs (bit-identical);
 *  12 = the patch kernel (6) as ONE persistent workgroup per CU: weight ring and patch buffers run on across tiles, register
 *       epilogue (layers eligible for 6 with cout >= 128 and no residual operand; the default on 28x28 / 14x14 maps; bit-identical to 6).
 *  16 = the grouped 3x3 kernel (csrc/mpx_gconv.h): one wave per 16 output pixels x channel block of max(cg, 16) channels, operands straight
 *       from global memory (the conv2 of a ResNeXt block: its only tile, and the tile of nothing else; ids 15 and 17 are unassigned).
 *  18 = the grouped 3x3 kernel for any group count, group widths 16 / 24 / 48 / 56 / 120 and planes at a pitch >= the width (csrc/mpx_gconvw.h): one
 *       wave per 32 output pixels x group x chunk of at most four 16-row fragments; it writes the output's pad channels as +0 itself (the
 *       f.b of a RegNetX / RegNetY block: its default; such a layer with 16 channels per group, a width that is a multiple of 64 and pitch = width also
 *       accepts tile 16, which gives the same bits.  Every layer that is not such a grouped layer is refused).
 * A tile a layer is not eligible for, or any other id, returns MPX_E_ARG; tile < 0 = the layer's default (a DenseNet's conv2, 3x3 128 -> 32,
 * defaults to 6, its topology's own choice: the cout <= 64 rule above was judged on 64 -> 64 layers and would give it 1).  (Ids 3, 5, 8 and 11 of
 * earlier rounds -- kernels that were measured and never became a default -- were removed; commit e4ccec8 is the last that has
 * them.)  A non-default tile on a layer of a block tail makes mpx_forward run that block layer by
 * layer (mpx_bottleneck_tail). */
int mpx_set_conv_tile(mpx_engine* h, int i, int tile);
int mpx_get_conv_tile(const mpx_engine* h, int i);
/* Test hook: which kernels the LAST mpx_conv_bn_act or mpx_conv_dual_bn_act call launched, as a bit mask over the tile ids above (bit t = the kernel of tile
 * t ran).  A layer's tile is a request: a launch under one round of tiles of a persistent kernel (10, 12, 13; 14: under two rounds) runs on the small-tile
 * kernel that sums in the same order (7, 6, 2; 14: 7), a residual operand sends 13 to 9, and the 256x256 kernels hand the images behind the
 * last whole round to tile 2 -- so a test that means to cover a persistent walk asserts that it ran. */
int mpx_last_conv_kernels(const mpx_engine* h);

/* Host-only packer (no GPU needed; what mpx_set_conv_weights runs before the upload).
 * Produces the fp16 planes w_hi/w_lo of cout_pad x k_packed elements (k order = (ky,kx,ci), ci fastest;
 * for a layer that reads the NHWC4 padded input -- cin == 3 and k_packed == ksize * 32: the ImageNet ResNets' 7x7 stem, the VGG first
 * layer -- k = ky*32 + px*4 + c, one run of 8 pixels x 4 channels per kernel row, zero weights on px >= ksize and c == 3; for AlexNet's
 * 11x11 first layer -- cin == 3, ksize == 11 and k_packed == 704 -- k = ky*64 + px*4 + c, one run of 16 pixels per kernel row) in PIECE-major order: element (row, k) of a plane is at
 *   ((((row/16) * (k_packed/32) + k/32) * 16 + row%16) * 4 + ((k/8)%4 ^ (((row%16)/8) * 2))) * 8 + k%8
 * -- [cout_pad/16][k_packed/32][16 rows][four 16-byte chunks, XOR-swizzled by the row], so that each 1-KiB LDS-DMA piece of
 * the conv kernels is one contiguous run of 8 cache lines already in the order of its LDS image (cout_pad % 16 == 0,
 * k_packed % 32 == 0).  Each output channel is
 * multiplied by 2^e so that max|w| lies in [512,1024), and the fp32 epilogue
 * scale = gamma/sqrt(var+eps) * 2^-e, shift = beta + (conv_bias - mean)*gamma/sqrt(var+eps).  k_packed = k*k*cin_pad
 * with cin_pad >= cin the channels per pixel of the input planes (padding channels get zero weights).
 * All outputs are HOST buffers sized from mpx_conv_desc (uint16_t = raw fp16 bits). */
int mpx_pack_conv_weights(const mpx_conv_desc* d, const float* w, const float* conv_bias, const float* gamma,
                          const float* beta, const float* mean, const float* var, float eps,
                          uint16_t* w_hi, uint16_t* w_lo, float* scale, float* shift);
/* ---- K0: mask-apply + normalise ----------------------------------------------------------
 * replaces: transforms.ToTensor + Normalize (generate_gp_training_data_imagenet.py:598-599),
 *           the per-segment pixel-mask build (:234-237), `input[0].numpy().copy() * mask`
 *           (:240) and the per-mask H2D copy (:242-245).
 * Exactly one of img_u8_hwc (DEV u8[224][224][3], raw pixels; normalised in-kernel as
 * (u8/255 - mean_c)/std_c in fp32) and img_f32_chw (DEV f32[3][224][224], already normalised,
 * what the reference's val_loader yields) is non-NULL.
 * seg: DEV i32[224][224], labels in [0,S) (rank in np.unique(segments) order).
 * onoff: DEV u8[M][S]; onoff[m][s] != 0 keeps superpixel s in mask m (normalise THEN mask:
 * removed pixels become 0.0 in normalised space).
 * Writes masked image m into engine input slot slot0+m (slot0+M <= max_batch) and, if
 * out_f32_nchw (DEV f32[M][3][224][224]) is non-NULL, the reference-layout tensor as well. */
int mpx_mask_apply_normalize(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw,
                             const int32_t* seg, const uint8_t* onoff, int M, int S,
                             const float mean[3], const float std[3], int slot0,
                             float* out_f32_nchw, void* stream);

/* ---- K0 + stem + max pool for the masks of ONE image, by superposition ---------------------------------------
 * replaces: the same lines as mpx_mask_apply_normalize (generate_gp_training_data_imagenet.py:598-599,234-245) AND the first
 *           `x = self.conv1(x); x = self.bn1(x); x = self.relu(x); x = self.maxpool(x)` of model(masked_img_tensor) (:246) for
 *           every mask of one image.  conv1 is linear and a mask is a union of superpixels, so conv1(x * mask_m) at an output pixel is
 *           the sum, over the superpixels its 7x7 window touches, of onoff[m][s] * (the window's taps inside s) -- terms that do not
 *           depend on the mask.  mpx_stem_table_build computes them once per image (one fp32 conv of the normalised image, taps
 *           bucketed by label; the table lives in the engine and holds one image at a time); mpx_stem_table_apply then writes
 *           relu(bn1(sum of the kept terms)) max-pooled 3x3 / 2 for M mask rows into the engine's pooled stem planes, slots
 *           [slot0, slot0 + M) -- no masked image is ever materialised.  Same arguments as mpx_mask_apply_normalize (img: exactly
 *           one of u8 HWC / f32 CHW; seg ranks in [0, S); onoff[m][s] != 0 keeps superpixel s), S <= 4096.  fp32 FMA chains in tap
 *           order instead of the MFMA stem's split-fp16 products: equal up to rounding (~1e-7 relative).
 * mpx_forward runs the B slots from the pooled planes when ALL of them were staged this way since they were last staged by
 * mpx_mask_apply_normalize, from the input staging when none was, and fails (MPX_E_STATE) on a mixed batch.
 * The table's device memory (160 MB, independent of max_batch) is allocated by the FIRST mpx_stem_table_build of an engine -- the one
 * allocation behind this boundary after mpx_create (an engine that only stages through mpx_mask_apply_normalize never holds it);
 * mpx_workspace_bytes includes it from then on, mpx_destroy frees it. */
int mpx_stem_table_build(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const int32_t* seg, int S,
                         const float mean[3], const float std[3], void* stream);
int mpx_stem_table_apply(mpx_engine* h, const uint8_t* onoff, int M, int S, int slot0, void* stream);

/* ---- K0 for real-valued per-pixel masks: explicit weights, or RISE's grids synthesised in the kernel ---------------------------
 * extends: mpx_mask_apply_normalize, whose masks are binary unions of superpixels (the reference's windows,
 *          generate_gp_training_data_imagenet.py:223-245), to a weight w_m(p) in place of `keep`: masked = normalised image * w_m, the
 *          other common masked-perturbation convention.  There is no reference line: the RISE entry follows Petsiuk, Das, Saenko, "RISE:
 *          Randomized Input Sampling for Explanation of Black-box Models" (BMVC 2018) -- a random s x s grid upsampled bilinearly and
 *          cropped at a random shift --, the explicit entry takes whatever the caller computed (soft-edged occlusion windows, ...).
 * img_u8_hwc / img_f32_chw, mean, std, slot0, out_f32_nchw: as mpx_mask_apply_normalize (exactly one image pointer; the u8 image is
 * normalised with K0's op sequence; channel 3 of the padded NHWC4 planes is written as zero, the 3-pixel border is not touched).
 * o = v * w is ONE fp32 multiply, then the hi / lo split (hi = f16(o), lo = f16(o - f32(hi))).  For w in {0, 1} the planes and
 * out_f32_nchw equal mpx_mask_apply_normalize's bit for bit, the -0.0 of a removed negative pixel included (hi -0.0, lo +0.0 in the
 * planes).  No masked image is materialised on the way.
 * mpx_softmask_apply: weights DEV f32[M][224][224].
 * mpx_rise_apply: cells DEV u8[M][s][s] (non-zero = keep), shift DEV i32[M][2] = (dy, dx), 2 <= s <= 32.  With cell = ceil(224 / s) and
 *   U = (s + 1) * cell the weight of pixel (y, x) is the bilinear upsampling of the grid to U x U with half-pixel centres
 *   (torch.nn.functional.interpolate(.., size=(U, U), mode="bilinear", align_corners=False)), cropped at (dy, dx), computed as
 *     Y = y + dy;  t = max((2Y + 1) * s - U, 0);  i0 = t / (2U);  r = t - i0 * 2U;  fy = float(r) / float(2U);  i1 = min(i0 + 1, s - 1)
 *     (the same along x: j0, j1, fx)
 *     w = (1 - fy) * ((1 - fx) * g[i0][j0] + fx * g[i0][j1]) + fy * ((1 - fx) * g[i1][j0] + fx * g[i1][j1])
 *   with integer t, i0, r, one correctly rounded fp32 division per axis, and every difference, product and sum of the last line rounded to
 *   fp32 on its own in the order written (products before their sum, no FMA): csrc/mpx_softmask.h, restated by masks.rise_weights.
 *   A shift outside [0, cell) is outside the contract and its result undefined (the kernels clamp it so that nothing is read out of
 *   bounds); the Python layer refuses it before upload.
 * Both mark slots [slot0, slot0 + M) as input-staged, as mpx_mask_apply_normalize does: mpx_forward runs the stem on them, and a batch
 * mixed with slots staged by mpx_stem_table_apply fails as it does today.  MPX_E_STATE on an engine of one of the small networks (their
 * convention is mpx_mask_apply_minmax's).  MPX_E_ARG, with nothing written, for s outside [2, 32], M < 0 or slot0 + M > max_batch, both
 * or neither image pointer, a NULL mask pointer.  M == 0 succeeds and writes nothing. */
int mpx_softmask_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* weights, int M,
                       const float mean[3], const float std[3], int slot0, float* out_f32_nchw, void* stream);
int mpx_rise_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const uint8_t* cells, const int32_t* shift,
                   int M, int s, const float mean[3], const float std[3], int slot0, float* out_f32_nchw, void* stream);

/* ---- the rows of a Sobol total-order design over a grid of cells, synthesised in the apply kernel ---------------------------------
 * extends: mpx_softmask_apply / mpx_rise_apply (a weight per pixel, the removed pixel always zero) to the perturbations of Fel, Cadene,
 *          Chalvidal, Cord, Vigouroux, Serre, "Look at the Variance! Efficient Black-box Explanations with Sobol-based Sensitivity
 *          Analysis" (NeurIPS 2021): the image is cut into d x d piecewise constant cells, every cell gets a weight in [0, 1] from a
 *          quasi-Monte-Carlo design, and a cell's total-order index is estimated from N * (d * d + 1) scores (Jansen's estimator).  There
 *          is no reference line.  The design is two matrices, and every row's 224 x 224 weights are gathered from them in the kernel
 *          (csrc/mpx_softmask.h, DesignWeights) instead of being uploaded.
 * A, B: DEV f32[N][D], D = d * d, 2 <= d <= 32 (MPX_SOBOL_GRID_MIN / _MAX), N >= 2.  The design has R = N * (D + 1) rows; row r is
 *     r <  N:  the cells are A[r]
 *     r >= N:  q = r - N, j = q / D, i = q - j * D: the cells are A[j] with cell i taken from B[j]        (j-major; B is no row of its own)
 * and the weight of pixel (y, x) under row r is the value of its cell c = ((y * d) / 224) * d + (x * d) / 224 (integer divisions): a pure
 * gather, no arithmetic.  The call stages rows [row0, row0 + M) into slots [slot0, slot0 + M).
 * img_u8_hwc / img_f32_chw, mean, std, slot0, out_f32_nchw: as mpx_softmask_apply.  fill_f32_chw: NULL, or DEV f32[3][224][224] in
 * normalised space (what mpx_blur_fill writes).  Per channel, with v the normalised pixel, w the weight and F the fill pixel:
 *     without a fill:  o = fl(v * w)                                    mpx_softmask_apply's planes for the same weights, bit for bit
 *     with a fill:     o = fl(fl(v * w) + fl(F * fl(1 - w)))            four fp32 operations, each rounded on its own, no FMA
 * then the hi / lo split, channel 3 = +0.0, the 3-pixel border untouched, out_f32_nchw[m][c][p] = o when given.
 * Values of A / B outside [0, 1] are outside the contract; nothing is clamped (the Python layer refuses them before upload).
 * Marks slots [slot0, slot0 + M) input-staged.  MPX_E_STATE on the small networks.  MPX_E_ARG, with nothing written, for d outside
 * [2, 32], N < 2, N * (D + 1) not representable in int, M < 0, row0 < 0, row0 + M > N * (D + 1), slot0 + M > max_batch, a NULL A or B,
 * both or neither image pointer.  M == 0 succeeds and writes nothing.  No allocation, no host synchronisation. */
#define MPX_SOBOL_GRID_MIN 2
#define MPX_SOBOL_GRID_MAX 32
int mpx_sobol_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* A, const float* B, int N, int d,
                    int row0, int M, const float* fill_f32_chw, const float mean[3], const float std[3], int slot0, float* out_f32_nchw,
                    void* stream);

/* ---- occlusion sensitivity: one sliding box per row, synthesised in the apply kernel; the overlap mean of the score drops ------------
 * extends: mpx_softmask_apply (a 200 KB weight map per row) to the oldest perturbation method -- Zeiler, Fergus, "Visualizing and
 *          Understanding Convolutional Networks" (ECCV 2014), Captum's Occlusion, MATLAB's occlusionSensitivity: a box slides over the
 *          image, the score with the box covered is compared with the score of the whole image, and every pixel gets the mean drop over
 *          the boxes that cover it.  There is no reference line.  A box is 16 bytes (csrc/mpx_softmask.h BoxWeights, csrc/mpx_occlusion.h).
 * mpx_box_apply: boxes DEV i32[M][4] = (y0, x0, y1, x1), half-open: pixel (y, x) is covered iff y0 <= y < y1 && x0 <= x < x1.  The contract
 *   is 0 <= y0 <= y1 <= 224 and 0 <= x0 <= x1 <= 224; an EMPTY box is legal and stages the unoccluded image.  The kernel compares against
 *   the four values and never indexes by them: a box outside the contract is memory-safe.  The weight is w = covered ? 0.0f : 1.0f and,
 *   per channel, with v the normalised pixel and F the fill pixel (fill_f32_chw: NULL, or DEV f32[3][224][224] in normalised space):
 *     without a fill:  o = fl(v * w)                              a covered negative pixel is -0.0, as in mpx_mask_apply_normalize
 *     with a fill:     o = fl(fl(v * w) + fl(F * fl(1 - w)))      mpx_sobol_apply's blend; as VALUES a select between v and F
 *   then the hi / lo split, channel 3 = +0.0, the 3-pixel border untouched, out_f32_nchw[m][c][p] = o when given: mpx_softmask_apply's
 *   planes for the same weights, bit for bit.  No fill is zero in normalised space, the ImageNet mean colour: Zeiler and Fergus's grey
 *   square.  img_u8_hwc / img_f32_chw, mean, std, slot0, out_f32_nchw: as mpx_softmask_apply.  Marks slots [slot0, slot0 + M)
 *   input-staged.  MPX_E_STATE on the small networks.  MPX_E_ARG, with nothing written, for a NULL boxes, both or neither image pointer,
 *   M < 0, slot0 < 0 or slot0 + M > max_batch (checked in 64 bits).  M == 0 succeeds and writes nothing.
 * mpx_box_saliency_classes: boxes as above; scores DEV f32[M][score_pitch], score_pitch >= K; base DEV f32[K], the scores of the
 *   unoccluded image (it may point into scores: both are only read); sum DEV f32[K][224][224] and cnt DEV i32[224][224], both accumulated
 *   in place from what they hold.  For m = 0 .. M - 1 in this order, for every pixel p that box m covers:
 *     sum[k][p] <- fl(sum[k][p] + fl(base[k] - scores[m * score_pitch + k]))        for every class k
 *     cnt[p]    <- cnt[p] + 1
 *   ONE rounded fp32 subtraction and ONE rounded fp32 addition; a box that does not cover p leaves sum[.][p] and cnt[p] unchanged.  One
 *   thread owns a pixel and a tile of classes and walks the boxes in order (no atomics, no reduction tree): the bits depend neither on the
 *   launch geometry nor on how the rows are cut into consecutive calls.  Nothing is read beyond scores[..][K) or base[K).
 * mpx_box_saliency_mean: out[k][p] = cnt[p] > 0 ? sum[k][p] / float(cnt[p]) : 0.0f, one correctly rounded fp32 division; out DEV
 *   f32[K][224][224] may be sum.
 * Both: MPX_E_STATE on the small networks; MPX_E_ARG, with nothing launched, for a NULL pointer, M < 0, K <= 0, score_pitch < K.
 * M == 0 succeeds and writes nothing.  No allocation, no host synchronisation. */
int mpx_box_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const int32_t* boxes, int M,
                  const float* fill_f32_chw, const float mean[3], const float std[3], int slot0, float* out_f32_nchw, void* stream);
int mpx_box_saliency_classes(mpx_engine* h, const int32_t* boxes, const float* scores, int score_pitch, const float* base, int M, int K,
                             float* sum, int32_t* cnt, void* stream);
int mpx_box_saliency_mean(mpx_engine* h, const float* sum, const int32_t* cnt, int K, float* out, void* stream);

/* ---- Score-CAM: the network's own activation maps as masks, upsampled in the apply kernel ------------------------------------------------
 * extends: mpx_softmask_apply (a 200 KB weight map per row) to the family of forward-only attributions whose masks come from inside the
 *          network -- Wang et al., "Score-CAM: Score-Weighted Visual Explanations for Convolutional Neural Networks" (CVPR-W 2020),
 *          ScoreCAM in pytorch-grad-cam: every channel of the last feature map is upsampled to the image, normalised to [0, 1] and scored
 *          as a mask; the class activation map is the sum of the channels weighted by their scores.  There is no reference line.  A row is
 *          g x g floats (csrc/mpx_softmask.h MapWeights, csrc/mpx_cam.h).
 * up(G)(y, x), G f32[g][g], 2 <= g <= 16 (MPX_CAM_GRID_MIN / _MAX): bilinear, half-pixel centres, g -> 224, one axis from integers
 *     t = max((2y + 1) * g - 224, 0);  i0 = t / 448;  r = t - 448 * i0;  f = fl(float(r) / 448.0f);  i1 = min(i0 + 1, g - 1)
 *     top = fl(fl(fl(1 - fx) * G[i0][j0]) + fl(fx * G[i0][j1])),  bot likewise on row i1,  up = fl(fl(fl(1 - fy) * top) + fl(fy * bot))
 *   every product and sum rounded on its own, no FMA: torch.nn.functional.interpolate(G, size=(224, 224), mode="bilinear",
 *   align_corners=False) up to rounding.  An all-ones grid gives exactly 1.0, an all-zeros grid exactly 0.0.
 * mpx_pool_input: a getter.  Where the global average pool of the op list the last mpx_forward ran (before any: the plain list) reads its
 *   input: DEV fp16 planes [max_batch][side * side][pitch], of which the first `channels` of every pitch are logical (channels = the input
 *   width of the logit layer behind the pool; the class count where the pool itself writes the logits), and what the pool applies to a
 *   value as it loads it: load = 0 nothing, 1 fminf(x, 6), 2 silu(x).  The planes hold the last forward's batch until the next forward.
 *   MPX_E_STATE, with a text that names the architecture, where the network has no such pool (the VGGs, AlexNet, ViT, the small networks).
 * mpx_planes_to_chw: out_f32 DEV f32[channels][side][side], out[c][cell] = LOAD(fl(f32(hi) + f32(lo))) of slot `slot` of explicit planes
 *   [.][side * side][pitch] (as mpx_global_avgpool takes them).  Pad channels [channels, pitch) are not read.  MPX_E_ARG for a NULL
 *   pointer, side outside [1, 224], channels < 0 or > pitch, load outside [0, 2], slot outside [0, max_batch).  channels == 0 succeeds and
 *   writes nothing.
 * mpx_cam_cells: act DEV f32[C][g][g] -> per channel c
 *     lo[c], hi[c] = min / max over all 224 x 224 pixels of up(act_c)           (the published code normalises the UPSAMPLED map)
 *     valid[c]     = (max cell > min cell) && (hi[c] > lo[c])                   u8, 1 / 0
 *     cells[c]     = fl(fl(act_c - lo[c]) / fl(hi[c] - lo[c]))                  one correctly rounded division; all +0.0 where !valid[c]
 *   cells DEV f32[C][g][g] lie slightly outside [0, 1] (an interior extreme is reached by no pixel centre).  min and max are exact.
 * mpx_cam_apply: cells DEV f32[M][g][g]; the weight of row m at pixel p is w = min(max(up(cells_m)(p), 0), 1) (as selects: a zero weight is
 *   +0.0), then mpx_softmask_apply's o = fl(v * w), the hi / lo split, channel 3 = +0.0, the 3-pixel border untouched,
 *   out_f32_nchw[m][c][p] = o when given: mpx_softmask_apply's planes for the same weights, bit for bit.  img_u8_hwc / img_f32_chw, mean,
 *   std, slot0, out_f32_nchw: as mpx_softmask_apply.  Marks slots [slot0, slot0 + M) input-staged.
 * mpx_cam_combine: act DEV f32[R][g][g] (the RAW activations of the scored rows), scores DEV f32[R][score_pitch], score_pitch >= K:
 *     low[k][cell] = +0.0, then for r = 0 .. R - 1 in this order  low[k][cell] <- fl(low[k][cell] + fl(scores[r * score_pitch + k] * act[r][cell]))
 *     sal[k][p]    = v > 0 ? v : +0.0  with  v = up(low[k])(p)
 *   low DEV f32[K][g][g] (the class activation map at layer resolution), sal DEV f32[K][224][224]; both are overwritten.  One thread owns a
 *   (class, cell) and walks the rows in order: no atomics, no reduction tree.  R == 0 writes zero maps (act and scores may be NULL then).
 * mpx_cam_cells / _apply / _combine: MPX_E_STATE on the small networks.  MPX_E_ARG, with nothing written or launched, for g outside
 * [2, 16], a NULL pointer, both or neither image pointer, M / R / C < 0, K <= 0, score_pitch < K, slot0 < 0 or slot0 + M > max_batch
 * (checked in 64 bits).  M == 0 / C == 0 succeed and write nothing.  No allocation, no host synchronisation. */
#define MPX_CAM_GRID_MIN 2
#define MPX_CAM_GRID_MAX 16
int mpx_pool_input(mpx_engine* h, void** hi, void** lo, int* side, int* channels, int* pitch, int* load);
int mpx_planes_to_chw(mpx_engine* h, const void* in_hi, const void* in_lo, int slot, int side, int channels, int pitch, int load,
                      float* out_f32, void* stream);
int mpx_cam_cells(mpx_engine* h, const float* act, int C, int g, float* cells, float* lo, float* hi, uint8_t* valid, void* stream);
int mpx_cam_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* cells, int M, int g, const float mean[3],
                  const float std[3], int slot0, float* out_f32_nchw, void* stream);
int mpx_cam_combine(mpx_engine* h, const float* act, const float* scores, int score_pitch, int R, int g, int K, float* low, float* sal,
                    void* stream);

/* ---- the score-weighted sum of real-valued masks (RISE's saliency map, before its normalisation) -------------------------------
 * extends: mpx_heatmap_accumulate (counts of binary masks) to  sal[p] <- sal[p] + weight[m] * w_m(p)  for m = 0 .. M - 1 in this order,
 *          accumulated in place in fp32 from the value already in sal (RISE's Monte Carlo estimate: the masks weighted by the class score).
 * Each step is a multiply and an add, each rounded to fp32 -- not an FMA.  One thread owns a pixel and walks the masks in order (no
 * atomics, no reduction tree): a pixel's bits depend neither on the launch geometry nor on how the rows are cut into consecutive calls.
 * weights / cells / shift / s: as the apply entries; weight DEV f32[M] (the scores of the forward that just ran); sal DEV f32[224][224].
 * MPX_E_STATE on the small networks, MPX_E_ARG for a NULL pointer, M < 0 or s outside [2, 32]; M == 0 succeeds and writes nothing. */
int mpx_softmask_saliency(mpx_engine* h, const float* weights, const float* weight, int M, float* sal, void* stream);
int mpx_rise_saliency(mpx_engine* h, const uint8_t* cells, const int32_t* shift, const float* weight, int M, int s, float* sal,
                      void* stream);

/* ---- many classes from the same forwards: K gathers per row of logits, and the saliency sum with a tile of classes per thread --------
 * extends: mpx_head_softmax_gather (one label per row) and mpx_softmask_saliency / mpx_rise_saliency (one weight per mask) to RISE's
 *          estimator as published, sal[k] = sum_m p_k(I * M_m) * M_m for every class k of the SAME forwards (csrc/mpx_saliency_classes.h).
 * mpx_softmax_gather_classes: logits DEV f32[B][logit_pitch] (mpx_forward's logits_out), classes DEV i32[K] or NULL (class k = k, and then
 *   K must be num_classes), scores DEV f32[B][score_pitch], score_pitch >= K.
 *     scores[b * score_pitch + k] = softmax(logits[b])[classes[k]]
 *   BIT FOR BIT what mpx_head_softmax_gather writes as score[b] for label[b] = classes[k]: one wave per row, lane l sums the terms
 *   expf(row[i] - max) of columns l, l + 64, .. in order, the lanes are reduced by xor-shuffles 32, 16, .., 1, the output is one correctly
 *   rounded division expf(row[c] - max) / sum.  A class outside [0, num_classes) gives 0.0f.  The padding [K, score_pitch) of a row is not
 *   written.  No argmax is returned (mpx_forward's pred is that).
 * mpx_softmask_saliency_classes / mpx_rise_saliency_classes: weights / cells / shift / s as the single-class entries, scores DEV
 *   f32[M][score_pitch], sal DEV f32[K][224][224].  For every class k and pixel p, for m = 0 .. M - 1 in this order, from the value
 *   already in sal:
 *     sal[k][p] <- fl(sal[k][p] + fl(scores[m * score_pitch + k] * w_m(p)))
 *   a multiply and an add, each rounded to fp32 -- not an FMA; w_m(p) is the weight of the apply entries.  Map k is BIT FOR BIT what
 *   mpx_softmask_saliency / mpx_rise_saliency leave in sal[k] when called with weight[m] = scores[m * score_pitch + k].  One thread owns a
 *   pixel and a tile of classes and walks the masks in order (no atomics, no reduction tree): the bits depend neither on the launch
 *   geometry nor on how the rows are cut into consecutive calls.  Nothing is read beyond scores[..][K) or written beyond sal[K).
 * All three: MPX_E_STATE on the small networks; MPX_E_ARG, with nothing launched, for a NULL pointer (classes excepted), B, M or K <= 0,
 * score_pitch < K, classes == NULL with K != num_classes, s outside [2, 32]. */
int mpx_softmax_gather_classes(mpx_engine* h, const float* logits, const int32_t* classes, int K, float* scores, int score_pitch, int B,
                               void* stream);
int mpx_softmask_saliency_classes(mpx_engine* h, const float* weights, const float* scores, int score_pitch, int M, int K, float* sal,
                                  void* stream);
int mpx_rise_saliency_classes(mpx_engine* h, const uint8_t* cells, const int32_t* shift, const float* scores, int score_pitch, int M,
                              int K, int s, float* sal, void* stream);

/* ---- a linear surrogate over on/off superpixel rows: the fp64 moment sums of LIME and KernelSHAP, and the paint per superpixel ---------
 * extends: mpx_heatmap_accumulate (one count per superpixel of the rows predicted right) to the two sums a weighted least-squares fit of
 *          score ~ c0 + sum_j c_j * z_j  over random on/off rows needs (Ribeiro et al., "LIME", KDD 2016; Lundberg & Lee, "KernelSHAP",
 *          NeurIPS 2017), for K classes of the same forwards (csrc/mpx_surrogate.h).  There is no reference line.
 * mpx_surrogate_accumulate: onoff DEV u8[M][S] (any non-zero byte = on), weight DEV f32[M], scores DEV f32[M][score_pitch] with
 *   score_pitch >= K (what mpx_softmax_gather_classes writes), A DEV f64[S+1][S+1], B DEV f64[S+1][K], both dense and row-major.
 *   With z~_m = (1, onoff[m][0] != 0, .., onoff[m][S-1] != 0), for m = 0 .. M - 1 in this order, from the values already in A and B:
 *     A[i][j] <- fl64(A[i][j] + (double)weight[m])                                          where z~_mi and z~_mj are both on
 *     B[i][k] <- fl64(B[i][k] + (double)weight[m] * (double)scores[m * score_pitch + k])    where z~_mi is on
 *   and an element whose condition is off is not touched.  The product of two fp32 numbers is exact in fp64, so every step has ONE
 *   rounding, and an FMA and a multiply-add give the same bits.  Both triangles of A are written.  The weight and the scores of a row reach
 *   only the elements whose condition that row turns on: a NaN on an off row reaches nothing, a NaN score of class k on an on row reaches
 *   column k of the rows of its on superpixels (and row 0).  One thread owns a row and a tile of columns and walks the masks in order (no
 *   atomics, no reduction tree): the bits depend neither on the launch geometry nor on how the rows are cut into consecutive calls.
 *   Nothing is read in scores[..][K, score_pitch), nothing is written outside A and B.  1 <= S <= 1024.
 * mpx_segment_paint: seg DEV i32[H][H] (H = the engine's image_size), value DEV f32[K][value_pitch] with value_pitch >= S,
 *   out DEV f32[K][H][H]:
 *     out[k][p] = value[k * value_pitch + seg[p]],   +0.0f where seg[p] lies outside [0, S)
 * Both serve every engine, the small networks included (neither depends on the network).  MPX_E_ARG, with nothing launched, for a NULL
 * pointer, M < 0, K < 1, S outside [1, 1024], score_pitch < K or value_pitch < S.  M == 0 succeeds and writes nothing.  No allocation, no
 * host synchronisation. */
int mpx_surrogate_accumulate(mpx_engine* h, const uint8_t* onoff, const float* weight, const float* scores, int score_pitch, int M, int S,
                             int K, double* A, double* B, void* stream);
int mpx_segment_paint(mpx_engine* h, const int32_t* seg, const float* value, int value_pitch, int S, int K, float* out, void* stream);

/* ---- a second pixel source for the staging: rows selected on a per-pixel rank, and the blurred image ------------------------------
 * extends: mpx_mask_apply_normalize and the soft-mask entries, whose removed pixel is always zero, to a FILL IMAGE: row m takes the pixels
 *          of rank below thresh[m] from one source and the others from the other.  There is no reference line: these are the rows of the
 *          deletion and insertion curves of Petsiuk, Das, Saenko, "RISE" (BMVC 2018), section 4.1 -- deletion replaces the most salient
 *          pixels by a substrate `step` at a time, insertion reveals them on a blurred image (csrc/mpx_rankmask.h).
 * mpx_rank_apply: img_u8_hwc / img_f32_chw, mean, std, slot0, out_f32_nchw as mpx_mask_apply_normalize (exactly one image pointer).
 *   rank DEV i32[224][224], thresh DEV i32[M], fill_f32_chw DEV f32[3][224][224] or NULL, keep_top 0 or 1.  Per row m, pixel p, channel c:
 *     V   = the normalised pixel, mpx_mask_apply_normalize's op sequence bit for bit (or the f32 as given)
 *     F   = fill[c][p], or, without a fill image, V * 0.0f: mpx_mask_apply_normalize's removed pixel, the -0.0 of a negative pixel included
 *     top = rank[p] < thresh[m]     (signed integer compare; nothing else is asked of rank or thresh: they need be no permutation)
 *     o   = keep_top ? (top ? V : F) : (top ? F : V)
 *   then the hi / lo split, channel 3 = +0.0, the 3-pixel border untouched, out_f32_nchw[m][c][p] = o when given.  No multiply touches a
 *   kept pixel.  Without a fill image and with keep_top = 0, rows of thresholds i * step equal mpx_mask_apply_normalize's planes over the
 *   pseudo-segments rank / step bit for bit.  Marks slots [slot0, slot0 + M) input-staged, as mpx_softmask_apply does.
 *   MPX_E_STATE on the small networks; MPX_E_ARG, with nothing written, for both or neither image pointer, a NULL rank or thresh, M < 0,
 *   slot0 + M > max_batch, keep_top outside {0, 1}.  M == 0 succeeds and writes nothing.
 * mpx_blur_fill: out[3][224][224] = the separable correlation of the normalised image with taps (HOST f32[klen], read during the call as
 *   mean / std are), zero padding, klen odd in [1, 31], r = klen / 2:
 *     h[c][y][x]   = sum over k = 0 .. klen-1 with 0 <= x + k - r < 224, k ascending, from +0.0:  acc = fl(acc + fl(taps[k] * V[c][y][x + k - r]))
 *     out[c][y][x] = the same along y over h
 *   every product and sum rounded to fp32 on its own (no FMA); h stays in fp32 in the LDS.  With Gaussian taps this is what RISE's
 *   insertion starts from (its Conv2d(3, 3, klen, padding = klen / 2) on the normalised tensor); the result is a fill image for
 *   mpx_rank_apply.  MPX_E_STATE on the small networks; MPX_E_ARG, with nothing written, for both or neither image pointer, a NULL taps or
 *   out, klen even or outside [1, 31], out_f32_chw == img_f32_chw.
 * Both: no allocation, no host synchronisation. */
int mpx_rank_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const int32_t* rank, const int32_t* thresh, int M,
                   const float* fill_f32_chw, int keep_top, const float mean[3], const float std[3], int slot0, float* out_f32_nchw,
                   void* stream);
int mpx_blur_fill(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* taps, int klen, const float mean[3],
                  const float std[3], float* out_f32_chw, void* stream);

/* ---- K0 of the small networks: the CIFAR / MNIST scorers' mask convention ---------------------------
 * replaces: the in-place min-max rescale of the picture to [0,255] (generate_gp_training_data_cifar.py:274-279,
 *           generate_gp_training_data_mnist.py:167-171), `mask.fill(255); mask[segments == segVal] = 0` for the SELECTED
 *           superpixels (:310-313 / :213-217), `masked_img = org_img * mask`, the second in-place min-max rescale and
 *           normalize_image = * f32(1/255) (:315-321 / :220-242, utils.py:92-94), and the per-mask H2D copy.
 * img_f32_chw: DEV f32[C][H][W] as the loader yields it; seg: DEV i32[H][W] ranks in [0,S), S <= 4096;
 * removed: DEV u8[M][S], removed[m][s] != 0 switches superpixel s OFF in mask m.  Writes input slots [slot0, slot0+M) and,
 * if out_f32_nchw (DEV f32[M][C][H][W]) is non-NULL, the network input in the reference's layout (bit-exact against the
 * NumPy arithmetic; a mask that removes every pixel gives NaN, as 0/0 does upstream). */
int mpx_mask_apply_minmax(mpx_engine* h, const float* img_f32_chw, const int32_t* seg, const uint8_t* removed,
                          int M, int S, int slot0, float* out_f32_nchw, void* stream);

/* ---- DownsampleB (models/resnet.py:64-74): AvgPool2d(2) on the identity + zero channels; planes
 * [B][hin][hin][cin_p] -> [B][hin/2][hin/2][cout_p] (channel counts as stored: multiples of 8, cout_p >= cin_p).
 * Output channels [cin_p, cout_p) are exact zeros in both planes.  MPX_E_ARG for planes that are not 16-byte aligned. */
int mpx_avgpool2_pad(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B,
                     int hin, int cin_p, int cout_p, void* stream);

/* ---- K1/K2: conv + BN (+ residual) (+ ReLU), one layer ------------------------------------
 * replaces: one nn.Conv2d -> nn.BatchNorm2d (-> `out += identity`) (-> nn.ReLU) group inside
 *           model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * in_hi|lo, res_hi|lo, out_hi|lo: DEV fp16 NHWC planes [B][h][w][c] (layer 0 reads the engine's padded
 * NHWC4 input staging instead: pass in_hi = in_lo = NULL).  res_* may be NULL.
 * For the last entry ("fc") out_hi/out_lo are ignored and out_f32 (DEV f32[B][1000]) is written;
 * for every other layer out_f32 must be NULL (a SqueezeNet engine has no such entry: its last conv, classifier.1, writes planes
 * [B][13][13][1000] and out_f32 must be NULL there too).
 * An input-slice layer (a stride-1 ShuffleNetV2 block's branch2.0; mpx_conv_in_slice): in_hi|lo is the BASE of the stage planes
 * [B][h][w][pitch]; the layer reads channels [offset, offset + k_packed) of every pixel and nothing else -- the SLICE precedent, on the input side.
 * An output-slice layer (a SqueezeNet expand conv, the last conv of a GoogLeNet branch; mpx_conv_out_slice): out_hi|lo is the BASE of the
 * concatenated planes [B][h][w][pitch]; the layer writes channels [offset, offset + cout) of every pixel (inception4d.branch4.1: 16 zero
 * channels more, up to the pitch) and nothing else; res_* must be NULL. */
int mpx_conv_bn_act(mpx_engine* h, int i, const void* in_hi, const void* in_lo,
                    const void* res_hi, const void* res_lo, void* out_hi, void* out_lo,
                    float* out_f32, int B, void* stream);

/* ---- K1 with the downsample branch fused in ---------------------------------------------------
 * replaces: `out = self.bn3(self.conv3(out)); identity = self.downsample(x); out += identity; out = self.relu(out)`
 *           of the first Bottleneck of a stage (torchvision resnet.py, reached through model(masked_img_tensor),
 *           generate_gp_training_data_imagenet.py:246) as ONE launch: the 1x1 conv3 and the 1x1 (strided) downsample
 *           conv are K-concatenated, with the two BatchNorm scales folded into the weight rows as ratios <= 1
 *           (s = max(|s3|,|sd|): out = relu(s*(W3*s3/s . t2 + Wd*sd/s . x) + shift3 + shiftd)), so the downsample
 *           output never goes to HBM.  i = index of the block's conv3 ("layerN.0.conv3"); in_* = its input planes
 *           [B][h][w][cin3], x_* = the block input planes [B][H][W][cin_ds] (H = h * stride).  mpx_forward uses this
 *           path by default; mpx_set_fusion(h, 0) makes it run the two convs separately (bit-different, same
 *           tolerance; for tests and ablation).  Fused planes are built once both layers have weights. */
int mpx_conv_dual_bn_act(mpx_engine* h, int i, const void* in_hi, const void* in_lo, const void* x_hi,
                         const void* x_lo, void* out_hi, void* out_lo, int B, void* stream);
/* mask bit 0: the downsample fusion above and the stem + max-pool fusion below; bit 1: the block tails of layer1
 * (mpx_bottleneck_tail; needs bit 0 as well); bit 2: the pointwise tails of layer2 (mpx_pointwise_tail; needs bit 0 as well).
 * mpx_create starts with 7; 0 = one launch per layer. */
int mpx_set_fusion(mpx_engine* h, int mask);

/* ---- the tail of a 64-channel bottleneck block in ONE launch ------------------------------------------------
 * replaces: `out = self.relu(self.bn2(self.conv2(out))); out = self.bn3(self.conv3(out)); out += identity; out = self.relu(out)`
 *           of a layer1 Bottleneck AND `out = self.relu(self.bn1(self.conv1(x)))` of the block that follows it (torchvision
 *           resnet.py, reached through model(masked_img_tensor), generate_gp_training_data_imagenet.py:246).  layer1 works on
 *           56x56 maps and is HBM-bound; layer by layer a block moves 16 units (64 channels x 4 B per pixel) through HBM, this
 *           launch 10.4: conv2's output never leaves the registers (its accumulators are conv3's MFMA operand), and the
 *           256-channel trunk is read once -- as the identity -- instead of twice, because the next block's conv1 runs on the
 *           output tile while it is still on chip.  Only the 64-channel conv2 input needs a one-pixel halo (everything after
 *           the 3x3 conv is pointwise).
 * i = index of the block's conv2 ("layer1.N.conv2"); mpx_num_bottleneck_tails / mpx_bottleneck_tail_info list the blocks
 * that have this path (ResNet-50/101/152: the three blocks of layer1; the last one produces layer2.0.conv1's output).
 * t1_*: conv2's input planes [B][56][56][64]; x_*: the block's identity planes [B][56][56][256] -- for a block with a
 * downsample branch (layer1.0) the BLOCK INPUT planes [B][56][56][64], the branch being K-concatenated as in
 * mpx_conv_dual_bn_act; out_*: block output [B][56][56][256]; next_*: the following conv1's output [B][56][56][64 or 128].
 * For the block with the downsample branch t1_hi = t1_lo = NULL makes the launch compute t1 itself: the block's own
 * `out = self.relu(self.bn1(self.conv1(x)))` (64 -> 64, 1x1) runs on the halo tile of the block input it has staged anyway, so
 * layer1.0 is ONE launch with one read of its 64-channel input and neither t1 nor t2 ever in memory (what mpx_forward does).
 * All four plane pairs must be distinct buffers (workgroups read t1's halo while others write).  Same arithmetic as the
 * layer-by-layer path up to fp32 summation order.  mpx_forward takes this path by default. */
int mpx_bottleneck_tail(mpx_engine* h, int i, const void* t1_hi, const void* t1_lo, const void* x_hi, const void* x_lo,
                        void* out_hi, void* out_lo, void* next_hi, void* next_lo, int B, void* stream);
int mpx_num_bottleneck_tails(const mpx_engine* h);
/* layer indices of tail k: its conv2, conv3, downsample conv (-1 if none) and the following block's conv1; any pointer may be NULL */
int mpx_bottleneck_tail_info(const mpx_engine* h, int k, int* conv2, int* conv3, int* downsample, int* next_conv1);

/* ---- the pointwise tail of a 128-channel bottleneck block in ONE launch ---------------------------------------
 * replaces: `out = self.bn3(self.conv3(out)); out += identity; out = self.relu(out)` of a plain layer2 Bottleneck (no downsample
 *           branch) AND `out = self.relu(self.bn1(self.conv1(x)))` of the block that follows it (torchvision resnet.py, reached
 *           through model(masked_img_tensor), generate_gp_training_data_imagenet.py:246).  Layer by layer the 512-channel trunk is
 *           written by conv3 and read straight back by the next conv1; here the next conv1 runs on the output tile while it is on
 *           chip, so the trunk is read once (as the identity) and written once.  Everything is pointwise: a tile is 128 consecutive
 *           pixels of the flat [B * 28 * 28] index, and a pixel's result does not depend on where its tile starts.
 * i = index of the block's conv3 ("layer2.N.conv3"); mpx_num_pointwise_tails / mpx_pointwise_tail_info list the pairs that have
 * this path (ResNet-50 / 101: layer2.1 and layer2.2; ResNet-152: layer2.1 .. layer2.6).
 * t2_*: conv3's input planes [B][28][28][128]; x_*: the block's identity planes [B][28][28][512]; out_*: block output
 * [B][28][28][512]; next_*: the following conv1's output [B][28][28][128] (the pairs are found by their channel counts and the map
 * side the two layers share, 28 in these networks; the kernel walks the flat pixel index).  All four plane pairs must be distinct buffers.  The launch
 * reads the packed weight planes of its two layers as they are (a reload of either is seen by the next launch).  Same arithmetic as
 * the layer-by-layer path up to fp32 summation order.  mpx_forward takes this path by default; a non-default tile on either layer of
 * a pair makes it run that pair layer by layer. */
int mpx_pointwise_tail(mpx_engine* h, int i, const void* t2_hi, const void* t2_lo, const void* x_hi, const void* x_lo,
                       void* out_hi, void* out_lo, void* next_hi, void* next_lo, int B, void* stream);
int mpx_num_pointwise_tails(const mpx_engine* h);
/* layer indices of pointwise tail k: its conv3 and the following block's conv1; either pointer may be NULL */
int mpx_pointwise_tail_info(const mpx_engine* h, int k, int* conv3, int* next_conv1);

/* ---- K3: maxpool 3x3 s2 p1 (nn.MaxPool2d inside the same forward), NHWC split planes ------
 * Taps outside the map are left out (-inf padding), so the merged output equals F.max_pool2d(merged, 3, 2, 1) for any sign.
 * hin even, c a multiple of 8.  MPX_E_ARG for planes that are not 16-byte aligned. */
int mpx_maxpool3x3s2(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi,
                     void* out_lo, int B, int hin, int c, void* stream);

/* ---- K3 of the VGG networks: maxpool 2x2 s2 (nn.MaxPool2d(2, 2)), NHWC split planes [B][hin][hin][c] -> [B][hin/2][hin/2][c].
 * replaces: every "M" of torchvision's VGG cfgs inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * Bit-exact: each output (hi, lo) is the pair of the input element with the largest hi + lo.  hin even, c a multiple of 8.
 * MPX_E_ARG for planes that are not 16-byte aligned. */
int mpx_maxpool2x2s2(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi,
                     void* out_lo, int B, int hin, int c, void* stream);

/* ---- K3 of AlexNet: maxpool 3x3 s2 without padding (nn.MaxPool2d(3, 2)), NHWC split planes [B][hin][hin][c] -> [B][ho][ho][c] with
 * ho = (hin - 3) / 2 + 1: every window lies inside the map.
 * replaces: the three MaxPool2d(kernel_size=3, stride=2) of torchvision's AlexNet inside model(masked_img_tensor)
 *           (generate_gp_training_data_imagenet.py:246).
 * Bit-exact for any sign: each output (hi, lo) is the pair of the window's element with the largest hi + lo, the first in row-major
 * order on a tie.  MPX_E_ARG for hin < 3, an even hin (floor mode is not part of the contract), c not a multiple of 8 and planes that
 * are not 16-byte aligned. */
int mpx_maxpool3x3s2p0(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi,
                       void* out_lo, int B, int hin, int c, void* stream);

/* ---- GoogLeNet: 3x3 max pool with ceil-mode size, windows clipped at the map's edge --------------------------
 * replaces: `nn.MaxPool2d(3, stride=2, ceil_mode=True)` (maxpool1 / 2 / 3) and `nn.MaxPool2d(3, stride=1, padding=1, ceil_mode=True)`
 *           (branch4.0 of every Inception module) of torchvision's googlenet.py inside model(masked_img_tensor)
 *           (generate_gp_training_data_imagenet.py:246).
 * in: DEV split planes [B][hin][hin][pitch]; out: [B][ho][ho][pitch] with ho = ceil((hin + 2 * pad - 3) / stride) + 1, minus one if the
 * last window would start at or beyond hin + pad (PyTorch's rule).  stride 1 or 2, pad 0 or 1, pitch a multiple of 8 (all of a pixel's
 * pitch is pooled, pad channels included).  Taps outside the map are left out, never read as zero.  Bit-exact for any sign: each output
 * (hi, lo) is the pair of a window element with the largest hi + lo, so the merged output equals F.max_pool2d(merged, 3, stride, pad, 1,
 * ceil_mode=True).  in and out must not overlap.  MPX_E_ARG for any other stride or pad, hin + 2 * pad < 3, a pitch that is not a
 * multiple of 8, B <= 0, a null pointer or planes that are not 16-byte aligned.  ONE launch. */
int mpx_maxpool3x3_clip(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin, int stride, int pad,
                        int pitch, void* stream);
/* The clipped pools of a GoogLeNet engine's forward, in order (12; 0 for every other engine), and pool k's map side, stride, pad and pitch
 * (any pointer may be NULL). */
int mpx_num_clip_pools(const mpx_engine* h);
int mpx_clip_pool_info(const mpx_engine* h, int k, int* hin, int* stride, int* pad, int* pitch);

/* ---- DenseNet: concat-append + BatchNorm + ReLU on split planes ---------------------------------------------
 * replaces: `torch.cat(features, 1)` of a dense block (torchvision densenet.py _DenseBlock.forward / _DenseLayer.bn_function) for ONE new
 *           feature and the `relu(norm(.))` that the next consumer applies to the concatenation -- the next layer's norm1 + relu1, a
 *           transition's norm + relu, or features.norm5 + F.relu -- inside model(masked_img_tensor)
 *           (generate_gp_training_data_imagenet.py:246).
 * fresh_hi|lo: DEV planes [npix][fresh_stride] whose first g channels are the new feature (NULL, NULL with g = 0: nothing to append).
 * raw_hi|lo:   DEV planes [npix][c_total], the block's raw concatenation; channels [c_old, c_old + g) receive the fresh (hi, lo) pairs bit
 *              for bit, no other element is written.
 * out_hi|lo:   DEV planes [npix][c_norm], dense: split(relu(scale[c] * (hi + lo) + shift[c])) of channels [0, c_norm) of the concatenation
 *              as it is after the append, in fp32 (hi + lo is exact; one multiply, one add, the re-split).  NULL, NULL with c_norm = 0 and
 *              scale = shift = NULL: append only.  scale / shift: DEV f32[c_norm] (mpx_norm_params).
 * With both, c_norm == c_old + g (the fresh channels are read once, from fresh_*); without fresh, c_norm <= c_total.  ONE launch either
 * way.  Every channel count and stride is a multiple of 8 and every pointer 16-byte aligned (16-byte accesses), npix > 0; else MPX_E_ARG.
 * The three plane pairs must not overlap.  Offsets are 64-bit. */
int mpx_concat_bn_relu(mpx_engine* h, const void* fresh_hi, const void* fresh_lo, int g, int fresh_stride, void* raw_hi, void* raw_lo,
                       int c_total, int c_old, const float* scale, const float* shift, void* out_hi, void* out_lo, int c_norm,
                       long long npix, void* stream);

/* ---- DenseNet transitions: average pool 2x2 s2 (nn.AvgPool2d(2, 2)), NHWC split planes [B][hin][hin][c] -> [B][hin/2][hin/2][c].
 * replaces: `pool` of torchvision's _Transition inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * Each output is split(0.25 * (((x00 + x01) + x10) + x11)) of the merged taps in fp32.  MPX_E_ARG for hin odd or <= 0, c not a
 * positive multiple of 8 and planes that are not 16-byte aligned. */
int mpx_avgpool2x2s2(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin, int c,
                     void* stream);

/* ---- MobileNetV2: depthwise 3x3 conv (pad 1, stride 1 or 2) + BatchNorm + ReLU6 on split planes ----------------------------------
 * replaces: one `Conv2dNormActivation(hidden, hidden, stride=stride, groups=hidden, activation_layer=nn.ReLU6)` of torchvision's
 *           InvertedResidual inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * in_hi|lo:  DEV planes [B][hin][hin][pitch]; out_hi|lo: DEV planes [B][ho][ho][pitch], ho = (hin - 1) / stride + 1, every channel of the
 *            pitch written.  w: DEV f32[9][pitch], tap-major (tap = ky * 3 + kx); scale / shift: DEV f32[pitch] (mpx_dwconv_params).
 * Per output element, in fp32: x = hi + lo (exact), min(x, 6) when clamp_in != 0; acc = 0, then acc = fma(w[tap], x[tap], acc) over the taps
 * in row-major order (ky, then kx), taps outside the map left out; fl(fl(scale * acc) + shift); min(max(., 0), 6); the re-split.
 * pitch a positive multiple of 8, stride 1 or 2, every pointer 16-byte aligned, else MPX_E_ARG.  The planes must not overlap.  Offsets are
 * 64-bit.  ONE launch. */
int mpx_dwconv3x3_bn_relu6(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* scale, const float* shift,
                           void* out_hi, void* out_lo, int B, int hin, int pitch, int stride, int clamp_in, void* stream);

/* ---- ShuffleNetV2: depthwise 3x3 conv (pad 1, stride 1 or 2) + BatchNorm, NO activation, on split planes ---------------------------
 * replaces: `nn.Conv2d(c, c, 3, stride, 1, groups=c, bias=False)` + `nn.BatchNorm2d(c)` of torchvision's shufflenetv2.py InvertedResidual
 *           (branch1.0 / .1 and branch2.3 / .4) inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * Operands and arithmetic are mpx_dwconv3x3_bn_relu6's without its two clamps: x = hi + lo (exact); acc = fma(w[tap], x[tap], acc) over the
 * taps inside the map in row-major order; fl(fl(scale * acc) + shift); the re-split.  Negative results and results above 6 pass through.
 * Channels with zero weights, scale and shift (the pitch's pads, the gaps of a two-half map) come out as exact zeros for finite inputs.
 * MPX_E_ARG for a null pointer, B <= 0, hin <= 0, a pitch that is not a positive multiple of 8, a stride other than 1 or 2 and pointers that
 * are not 16-byte aligned.  The planes must not overlap.  Offsets are 64-bit.  ONE launch. */
int mpx_dwconv3x3_bn(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* scale, const float* shift,
                     void* out_hi, void* out_lo, int B, int hin, int pitch, int stride, void* stream);

/* ---- EfficientNet-B0: depthwise k x k conv (k = 3 or 5, pad (k - 1) / 2, stride 1 or 2) + BatchNorm with SiLU on either side ---------------
 * replaces: `Conv2dNormActivation(expanded, expanded, kernel_size=k, stride=stride, groups=expanded, activation_layer=nn.SiLU)` of torchvision's
 *           efficientnet.py MBConv AND the nn.SiLU of the Conv2dNormActivation in front of it (the expand conv; the stem for block 1.0),
 *           inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * in_hi|lo:  DEV planes [B][hin][hin][pitch]; out_hi|lo: DEV planes [B][ho][ho][pitch], ho = (hin - 1) / stride + 1, every channel of the
 *            pitch written.  w: DEV f32[ksize^2][pitch], tap-major (tap = ky * ksize + kx); scale / shift: DEV f32[pitch] (mpx_dwconv_params).
 * Per output element, in fp32: x = hi + lo (exact); a = act_in ? silu(x) : x with silu(x) = x / (1 + expf(-x)), the accurate expf and an IEEE
 * division; acc = 0, then acc = fma(w[tap], a[tap], acc) over the taps inside the map in row-major order; v = fl(fl(scale * acc) + shift);
 * act_out ? silu(v) : v; the re-split.  Channels with zero weights, scale and shift come out as exact zeros.  Act codes: 0 none, 1 SiLU.
 * MPX_E_ARG for ksize not 3 or 5, stride not 1 or 2, an act code other than 0 / 1, a pitch that is not a positive multiple of 8, a null or
 * misaligned (16 bytes) pointer, B <= 0 or hin <= 0.  The planes must not overlap.  Offsets are 64-bit.  ONE launch. */
int mpx_dwconv_bn_act(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* scale, const float* shift,
                      void* out_hi, void* out_lo, int B, int hin, int pitch, int ksize, int stride, int act_in, int act_out, void* stream);

/* ---- EfficientNet-B0: the Squeeze-and-Excitation gate, gate = sigmoid(fc2(silu(fc1(mean over the map)))) per image ----------------------
 * replaces: `scale = self.avgpool(input); scale = self.fc1(scale); scale = self.activation(scale); scale = self.fc2(scale); return
 *           self.scale_activation(scale)` (torchvision ops/misc.py SqueezeExcitation._scale with activation SiLU) inside
 *           model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * in_hi|lo: DEV planes [B][hw][pitch] (hw = PIXELS per image); gate: DEV f32[B][pitch].  w1: DEV f32[q][pitch]; b1: DEV f32[q]; w2: DEV
 * f32[q][pitch], j-major (w2[j][c] multiplies s1[j] into channel c); b2: DEV f32[pitch] (mpx_se_params).  Per image, in fp32:
 *     pooled[c] = (sum over the hw pixels of hi + lo) / hw;  s1[j] = silu(b1[j] + sum_c w1[j][c] pooled[c]), j < q;
 *     gate[c] = 1 / (1 + expf(-(b2[c] + sum_j w2[j][c] s1[j]))).
 * A pad channel carries zero w1 / w2 columns and b2 = -inf: its gate is 1 / (1 + inf) = 0 exactly.  One workgroup per image; every summation
 * order is a fixed function of (hw, pitch, q) -- never of B, the grid or timing, and there are no atomics --, so an image's gate has the same
 * bits alone and at any position of any batch.  hw >= 1, q >= 1 (no multiple of anything).  MPX_E_ARG for a null or misaligned (16 bytes)
 * pointer, B <= 0, hw <= 0, q <= 0, a pitch that is not a positive multiple of 8, or (pitch, q) whose LDS need passes 64 KB.  ONE launch. */
int mpx_se_gate(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w1, const float* b1, const float* w2, const float* b2,
                float* gate, int B, int hw, int pitch, int q, void* stream);

/* ---- EfficientNet-B0: the Squeeze-and-Excitation scale, out = split(fl((hi + lo) * gate[n][c])) ---------------------------------------
 * replaces: `return scale * input` of torchvision's SqueezeExcitation.forward inside model(masked_img_tensor)
 *           (generate_gp_training_data_imagenet.py:246).
 * in_hi|lo, out_hi|lo: DEV planes [B][hw][pitch] (hw = pixels per image); gate: DEV f32[B][pitch].  Element-wise: one fp32 multiply of the
 * exact hi + lo, the re-split.  out may be in (mpx_forward scales in place); any other overlap is undefined.  Same argument discipline as
 * mpx_se_gate.  ONE launch. */
/* ---- RegNetY: the Squeeze-and-Excitation gate with ReLU, gate = sigmoid(fc2(relu(fc1(mean over the map)))) per image --------------------
 * replaces: torchvision's SqueezeExcitation._scale with its default activation ReLU (regnet.py: ResBottleneckBlock's f.se) inside
 *           model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * mpx_se_gate in every respect -- operands, layouts, summation orders, the exact +0 gates of the pad channels, the refusals, ONE launch -- but
 * for fc1's activation: s1[j] = (v <= 0 ? 0 : v) with v = b1[j] + sum_c w1[j][c] pooled[c]. */
int mpx_se_gate_relu(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* gate, int B, int hw, int pitch, int q, void* stream);

int mpx_se_scale(mpx_engine* h, const void* in_hi, const void* in_lo, const float* gate, void* out_hi, void* out_lo, int B, int hw, int pitch,
                 void* stream);

/* ---- RegNetX / RegNetY: the any-width grouped 3x3 kernel (tile 18) on the caller's planes -------------------------------------------------
 * replaces: `self.b = Conv2dNormActivation(w_b, w_b, kernel_size=3, stride=stride, groups=g, ...)` of torchvision's BottleneckTransform
 *           (regnet.py) inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246), outside any engine's layer list.
 * mpx_pack_gconvw_weights (HOST, no engine): torchvision's weight [width][cg][3][3] (cg = width / groups = 16, 24, 48, 56 or 120) and the
 * BatchNorm vectors [width] -> the packed planes of csrc/mpx_gconvw.h, w_hi | w_lo: groups * ceil(cg / 16) * 16 rows of K = 9 cg rounded up
 * to 32 fp16 bit patterns each, scale | shift: one float per ROW (indexed by the channel; the tail zero).  MPX_E_ARG for anything else.
 * mpx_gconvw3x3_bn_act: in_hi|lo DEV planes [B][hin][hin][in_pitch], out_hi|lo DEV planes [B][hout][hout][out_pitch] (hout = (hin - 1) /
 * stride + 1; pad 1), w_hi|lo, scale, shift DEV copies of what the packer wrote.  The channels [width, out_pitch) of every output pixel are
 * written as +0; those of the input are never read.  groups = 1 is served here (one unit: three of a workgroup's four waves exit); an engine
 * layer of one group is an ordinary dense layer instead.  An output element's bits depend on its own pixel and group alone: not on B, the
 * image's index or the grid.  MPX_E_ARG for a null or misaligned (16 bytes) pointer, B <= 0, hin <= 0, a stride other than 1 or 2, a width
 * that is no multiple of groups, another group width, a pitch below the width or no multiple of 8.  ONE launch; mpx_last_conv_kernels = 1 << 18. */
int mpx_pack_gconvw_weights(int width, int groups, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                            float eps, uint16_t* w_hi, uint16_t* w_lo, float* scale, float* shift);
int mpx_gconvw3x3_bn_act(mpx_engine* h, const void* in_hi, const void* in_lo, const void* w_hi, const void* w_lo, const float* scale,
                         const float* shift, void* out_hi, void* out_lo, int B, int hin, int width, int groups, int in_pitch, int out_pitch,
                         int stride, int relu, void* stream);

/* ---- ConvNeXt: the LayerNorm over the channels of a pixel, alone and fused ---------------------------------------------------------
 * THE ARITHMETIC all three entries share, per pixel with channel values v_c, in fp32 with one rounding per operator (csrc/mpx_cnext.h):
 *     mean = (sum_c v_c) / C;  d_c = v_c - mean;  var = (sum_c d_c * d_c) / C  (two-pass: centred and biased, never E[v^2] - mean^2);
 *     rstd = 1 / sqrt(var + eps)  (IEEE square root and division);  y_c = ((d_c * rstd) * weight_c) + bias_c;  the re-split.
 * Both sums run in ONE fixed order -- the 8 channels of a 16-byte group ascending, then the C / 8 groups ascending --, through the LDS and
 * without atomics, so a pixel's result has the same bits in any batch, at any position of it and on any grid.  weight / bias: DEV f32[C].
 * C a positive multiple of 8 up to 2048; every pointer 16-byte aligned; the planes must not overlap; offsets are 64-bit.  max_blocks > 0 caps
 * the grid (a test hook: the result does not depend on it), 0 = the entry's own cap.  ONE launch each. */
/* replaces: `block.0` = nn.Conv2d(dim, dim, 7, padding=3, groups=dim, bias=True), the Permute and `block.2` = nn.LayerNorm(dim, eps=1e-6) of
 *           torchvision's convnext.py CNBlock inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * in / out: DEV planes [B][hin][hin][C].  w: DEV f32[49][C], tap-major (tap = ky * 7 + kx); conv_bias: DEV f32[C] (mpx_dwconv_params,
 * mpx_dwconv_ln).  v_c = acc_c + conv_bias_c with acc_c = fma(w[tap][c], x[tap][c], acc_c) over the taps inside the map in row-major order
 * from acc_c = 0, x = hi + lo (exact); v is never rounded to split-fp16 and never stored.  MPX_E_ARG for ksize != 7 (a 3x3 / 5x5 layer runs
 * mpx_dwconv_bn_act), stride != 1, a null or misaligned pointer, B <= 0, hin <= 0, C not a multiple of 8 or above 2048. */
int mpx_dwconv7x7_ln(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* conv_bias, const float* ln_weight,
                     const float* ln_bias, float eps, void* out_hi, void* out_lo, int B, int hin, int C, int ksize, int stride, int max_blocks,
                     void* stream);
/* replaces: a LayerNorm2d(C, eps=1e-6) of torchvision's convnext.py (features.0.1, features.2.0 / .4.0 / .6.0) inside model(masked_img_tensor).
 * in / out: DEV planes [rows][C], rows = B * h * w pixels; v_c = hi + lo (exact). */
int mpx_layernorm_c(mpx_engine* h, const void* in_hi, const void* in_lo, const float* ln_weight, const float* ln_bias, float eps, void* out_hi,
                    void* out_lo, long long rows, int C, int max_blocks, void* stream);
/* replaces: `self.avgpool(x)` (AdaptiveAvgPool2d(1)) and `classifier.0` = LayerNorm2d(768, eps=1e-6) of torchvision's ConvNeXt.
 * in: DEV planes [B][hw][C] (hw = PIXELS per image); out: DEV planes [B][C], what classifier.2 reads.  v_c = (the hw values hi + lo summed in
 * pixel order in fp32, mpx_global_avgpool's order) / hw, not re-split before the LayerNorm. */
int mpx_global_avgpool_ln(mpx_engine* h, const void* in_hi, const void* in_lo, const float* ln_weight, const float* ln_bias, float eps,
                          void* out_hi, void* out_lo, int B, int hw, int C, void* stream);

/* ---- ViT: scaled-dot-product attention, the token assembly, LayerNorm of strided rows ----------------------------------------------
 * replaces: `self.self_attention(x, x, x, need_weights=False)` of torchvision's vision_transformer.py EncoderBlock.forward BEHIND its input
 *           projection -- the softmax(Q K^T / 8) V of every head -- inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * qkv: DEV split planes [B][T][3 D], D = heads * 64 (head_dim is 64): Q at channel 0, K at D, V at 2 D, head h owning channels 64 h .. 64 h + 63
 * of each -- what in_proj writes.  out: DEV split planes [B][T][D], what out_proj reads.  Both products run on the fp16 MFMA pipe as the three
 * products A_hi B_lo, A_lo B_hi, A_hi B_hi into fp32.  THE CONTRACT per query row i of one (image, head), fp32, one rounding per operator
 * (csrc/mpx_attn.h):
 *     s_ij = 0.125f * (q_i . k_j);  m_i = max_j s_ij;  e_ij = expf(s_ij - m_i);
 *     l_i = ((part_0 + part_1) + part_2) + part_3 with part_g = the e_ij of the keys with (j >> 2) & 3 == g summed in ascending j;
 *     o_id = (sum_j split(1024 e_ij) v_jd) / (1024 l_i): one IEEE division per element behind the whole sum; the re-split.
 * Keys j >= T of the last step of 32 contribute exactly nothing (zero operands, the constant 0.f for e, no part in the maximum); query rows
 * >= T are never written.  An output row's bits depend on its image's data alone: not on B, the image's position in the batch or the grid.
 * MPX_E_ARG with a message for T < 1 or T > 512, heads outside 1 .. 64 (the width IS heads * 64), B <= 0, a null or misaligned (16 bytes) plane.
 * max_blocks > 0 caps the grid (a test hook: the result does not depend on it), 0 = the entry's own cap.  ONE launch. */
int mpx_attention(mpx_engine* h, const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, int B, int T, int heads, int max_blocks,
                  void* stream);
/* replaces: `torch.cat([batch_class_token, x], dim=1)` of VisionTransformer.forward and `input + self.pos_embedding` of Encoder.forward.
 * patch: DEV split planes [B][T - 1][D] (conv_proj's output); class_token: DEV f32[D]; pos_embedding: DEV f32[T][D] (mpx_token_params);
 * out: DEV split planes [B][T][D].  out[b][0] = class_token + pos[0], out[b][1 + i] = (hi + lo of patch[b][i], exact) + pos[1 + i]: one fp32 add
 * each, re-split.  MPX_E_STATE on an engine that is no ViT; MPX_E_ARG for T < 1, D no positive multiple of 8, a null or misaligned pointer. */
int mpx_tokens_assemble(mpx_engine* h, const void* patch_hi, const void* patch_lo, const float* class_token, const float* pos_embedding,
                        void* out_hi, void* out_lo, int B, int T, int D, int max_blocks, void* stream);
/* replaces: `self.ln(...)` of Encoder.forward as far as `x[:, 0]` reads it: the LayerNorm of input rows that lie in_stride rows apart.
 * in: DEV split planes [rows * in_stride][C] of which row r * in_stride is read; out: DEV split planes [rows][C].  mpx_layernorm_c's contract
 * unchanged (it is that kernel with a row stride on its loads); in_stride = T normalises the class-token row of each of `rows` images. */
int mpx_layernorm_rows(mpx_engine* h, const void* in_hi, const void* in_lo, const float* ln_weight, const float* ln_bias, float eps, void* out_hi,
                       void* out_lo, long long rows, long long in_stride, int C, int max_blocks, void* stream);
/* The attention launches of the op list in forward order (12 on a ViT engine, 0 on every other). */
typedef struct mpx_attn_desc {
    char name[48];       /* the module's state_dict prefix without "encoder.layers.": "encoder_layer_3.self_attention" */
    int32_t tokens;      /* T */
    int32_t heads;
    int32_t head_dim;    /* 64 */
} mpx_attn_desc;
int mpx_num_attn(const mpx_engine* h);
int mpx_attn_info(const mpx_engine* h, int k, mpx_attn_desc* out);
/* A ViT engine's two parameters that belong to no layer: HOST f32 class_token [1][1][D] and encoder.pos_embedding [1][T][D], uploaded
 * synchronously as they are; mpx_weights_complete and mpx_forward count them.  MPX_E_STATE on an engine that is no ViT.  mpx_token_params
 * returns their DEV pointers, T and D (NULL, NULL, 0, 0 on every other engine); any pointer may be NULL. */
int mpx_load_tokens(mpx_engine* h, const float* class_token, const float* pos_embedding);
int mpx_token_params(const mpx_engine* h, const float** class_token, const float** pos_embedding, int* tokens, int* width);

/* ---- ShuffleNetV2: channel_shuffle(cat(a, b), 2) into the two-half layout ------------------------------------------------------
 * replaces: `torch.cat((x1, self.branch2(x2)), dim=1)` / `torch.cat((self.branch1(x), self.branch2(x)), dim=1)` and `channel_shuffle(out, 2)`
 *           of torchvision's shufflenetv2.py InvertedResidual.forward inside model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).
 * a: DEV split planes [B][hw][hw][a_pitch], b: [B][hw][hw][b_pitch], bf real channels each (their other channels are never read); out:
 * [B][hw][hw][2 hp].  For physical output channel q, h = q / hp and j = q % hp: j >= bf gets zero bits in both planes; else l = h * bf + j and
 * the (hi, lo) pair is copied verbatim from (l & 1 ? b : a)[l >> 1].  Bit-exact.  a may be the first half of a two-half map (a_pitch = 2 hp)
 * and b its second half (pointer + hp, b_pitch = 2 hp).  out must not overlap a or b.
 * MPX_E_ARG for a null pointer, B <= 0, hw <= 0, bf odd or <= 0, hp < bf or not a multiple of 32, a pitch below bf or not a multiple of 8,
 * and pointers that are not 16-byte aligned.  Offsets are 64-bit.  ONE launch. */
int mpx_shuffle2_concat(mpx_engine* h, const void* a_hi, const void* a_lo, int a_pitch, const void* b_hi, const void* b_lo, int b_pitch,
                        void* out_hi, void* out_lo, int B, int hw, int bf, int hp, void* stream);
/* The shuffles of a ShuffleNetV2 engine's forward, in order (16; 0 for every other engine), and shuffle k's map side, bf, hp and the pitches
 * of its two sources (any pointer may be NULL). */
int mpx_num_shuffles(const mpx_engine* h);
int mpx_shuffle_info(const mpx_engine* h, int k, int* hw, int* bf, int* hp, int* a_pitch, int* b_pitch);

/* ---- MobileNetV2: K4a with the ReLU6 clamp of its producer: global average pool of min(x, 6), [B][hw][c] -> [B][c].
 * replaces: the ReLU6 of features.18 and `nn.functional.adaptive_avg_pool2d(x, (1, 1))` of torchvision's MobileNetV2 inside
 *           model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).  Sums in pixel order in fp32, divides by hw, re-splits;
 *           mpx_global_avgpool is unchanged.  c a multiple of 8. */
int mpx_global_avgpool_clamp6(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hw,
                              int c, void* stream);

/* ---- EfficientNet-B0: K4a with the SiLU of its producer: global average pool of silu(x), [B][hw][c] -> [B][c].
 * replaces: the nn.SiLU of features.8 and `self.avgpool(x)` (AdaptiveAvgPool2d(1)) of torchvision's EfficientNet inside
 *           model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).  silu(hi + lo) summed in pixel order in fp32, one division
 *           by hw, the re-split; mpx_global_avgpool is unchanged.  c a multiple of 8, planes 16-byte aligned. */
int mpx_global_avgpool_silu(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hw, int c,
                            void* stream);

/* ---- SqueezeNet: the global average pool that ends the network, [B][hw][c] split planes -> fp32 logits [B][out_pitch].
 * replaces: `nn.AdaptiveAvgPool2d((1, 1))` of torchvision's SqueezeNet classifier and the torch.flatten behind it inside
 *           model(masked_img_tensor) (generate_gp_training_data_imagenet.py:246).  Per channel: the hw values hi + lo summed in fp64 (exact: every
 *           value is a multiple of 2^-24), divided by hw in fp64 and rounded to fp32; written as fp32, which is what mpx_head_softmax_gather reads.
 *           Channels [c, out_pitch) of a row are left untouched.  mpx_global_avgpool is unchanged.
 * MPX_E_ARG for a null pointer, B <= 0, hw <= 0, c not a positive multiple of 8, out_pitch < c or planes that are not 16-byte aligned.
 * ONE launch. */
int mpx_global_avgpool_logits(mpx_engine* h, const void* in_hi, const void* in_lo, float* out_f32, int B, int hw, int c, int out_pitch,
                              void* stream);

/* ---- K1 + K3 in one launch: the ImageNet stem and its max pool -------------------------------------------
 * replaces: `x = self.conv1(x); x = self.bn1(x); x = self.relu(x); x = self.maxpool(x)` (torchvision resnet.py, reached through
 *           model(masked_img_tensor), generate_gp_training_data_imagenet.py:246): the 7x7 stride-2 conv + BN + ReLU of layer 0 reads
 *           the engine's own staged input (mpx_mask_apply_normalize) like mpx_conv_bn_act(h, 0, ...) and writes the POOLED planes
 *           [B][56][56][64]; a workgroup computes the 15 x 17 conv outputs under a 7 x 8 block of pooled pixels, so the 112 x 112 conv
 *           output (3.2 MB per image) is never written nor re-read.  Bit-identical to mpx_conv_bn_act + mpx_maxpool3x3s2.
 *           mpx_forward uses it by default (ImageNet ResNets, stem on its default tile); mpx_set_fusion(h, 0) turns it off together
 *           with the downsample fusion. */
int mpx_stem_conv_maxpool(mpx_engine* h, void* out_hi, void* out_lo, int B, void* stream);

/* ---- K4a: global average pool [B][hw][c] -> [B][c] (nn.AvgPool2d(7) + view) ----------------
 * hi + lo summed in pixel order in fp32, one division by hw, the re-split.  c a multiple of 8.  MPX_E_ARG for B * (c / 8) above
 * 2^31 - 1 and for planes that are not 16-byte aligned. */
int mpx_global_avgpool(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi,
                       void* out_lo, int B, int hw, int c, void* stream);

/* ---- K4b: softmax + gather(label) + argmax ------------------------------------------------
 * replaces: F.softmax(mask_output) ... [0][label] (bayesian_active_learning_imagenet.py:196-198)
 *           and mask_output.data.max(1, keepdim=True)[1] (generate_gp_training_data_imagenet.py:248).
 * logits DEV f32[B][1000]; label DEV i32[B]; score DEV f32[B]; pred DEV i32[B]. */
int mpx_head_softmax_gather(mpx_engine* h, const float* logits, const int32_t* label,
                            float* score, int32_t* pred, int B, void* stream);

/* ---- whole network -------------------------------------------------------------------------
 * replaces: mask_output = model(masked_img_tensor) + score extraction for B masked images
 *           already staged in input slots [0,B) by mpx_mask_apply_normalize.
 * logits_out (DEV f32[B][1000]) may be NULL. */
int mpx_forward(mpx_engine* h, const int32_t* label, float* score, int32_t* pred,
                float* logits_out, int B, void* stream);

/* ---- K5: heat-map accumulation ---------------------------------------------
 * replaces: summed_superpixel_labels[segments == v] += 1 for every selected superpixel of a correctly
 *           predicted mask (gp_superpixel_data_imagenet.py:322-323) and the pure-Python read-back loops of
 *           gp_regression.py:82-94:  heat[p] += sum_m [pred[m] == label[m]] * onoff[m][seg[p]].
 * seg DEV i32[224][224] ranks, onoff DEV u8[M][S], pred/label DEV i32[M], heat DEV f32[224][224] (accumulated
 * in place: zero it first; with several GPUs all-reduce it afterwards).  Uses a small engine-owned scratch
 * (S <= 4096). */
int mpx_heatmap_accumulate(mpx_engine* h, const int32_t* seg, const uint8_t* onoff, const int32_t* pred,
                           const int32_t* label, int M, int S, float* heat, void* stream);

/* ---- introspection for tests / benchmarks --------------------------------------------------- */
/* DEV pointers of the input staging planes: fp16 [max_batch][230][230][4] (padded NHWC4) for the ImageNet ResNets, VGG and AlexNet, [max_batch][H][W][32] for
 * the small networks.  A pure getter: the record of how each slot was staged is not touched, so a diagnostic call between
 * mpx_stem_table_apply and mpx_forward changes nothing. */
int mpx_input_planes(const mpx_engine* h, void** hi, void** lo);
/* A caller that has WRITTEN the input planes of slots [slot0, slot0+M) by hand declares them staged, as mpx_mask_apply_normalize does for the
 * slots it fills: the next mpx_forward runs the stem conv + max pool on them even if an earlier batch of the same slots came from
 * mpx_stem_table_apply (which marks the slots it writes as its own again).  MPX_E_ARG outside [0, max_batch). */
int mpx_mark_input_staged(mpx_engine* h, int slot0, int M);
/* DEV pointers of the pooled stem output planes: fp16 [max_batch][56][56][64], written by the stem + max pool launch of mpx_forward or by
 * mpx_stem_table_apply (NULL for the small networks, VGG and AlexNet, which have no such stem). */
int mpx_stem_planes(const mpx_engine* h, void** hi, void** lo);
/* When enabled, every kernel launch of mpx_forward / mpx_mask_apply_normalize is bracketed by
 * HIP events on the launch stream (bounded pool; launches beyond it are not recorded). */
int mpx_profile_enable(mpx_engine* h, int on);
/* Synchronises the recorded events, ADDS their durations into the caller's arrays and clears
 * the pool.  kind: 0 = conv (K1/K2), 1 = mask_apply_normalize (K0), 2 = pools (K3/K4a),
 * 3 = head (K4b).  per_conv_ms (HOST f64[mpx_num_convs], may be NULL) gets the per-layer split. */
int mpx_profile_collect(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4],
                        double* per_conv_ms);
/* The same with the split of kind 2 that a DenseNet engine adds: per_norm_ms (HOST f64[mpx_num_norms], may be NULL) gets the
 * mpx_concat_bn_relu launch of every stand-alone BatchNorm, avgpool2_ms (HOST f64[1], may be NULL) the transitions' average pools. */
int mpx_profile_collect_ex(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                           double* per_norm_ms, double* avgpool2_ms);
/* The same with MobileNetV2's split of kind 2: per_dw_ms (HOST f64[mpx_num_dwconvs], may be NULL) gets the launch of every depthwise
 * layer. */
int mpx_profile_collect_dw(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                           double* per_norm_ms, double* avgpool2_ms, double* per_dw_ms);
/* The same with GoogLeNet's split of kind 2: per_clip_pool_ms (HOST f64[mpx_num_clip_pools], may be NULL) gets every clipped max pool
 * launch of the forward. */
int mpx_profile_collect_pool(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                             double* per_norm_ms, double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms);
/* The same with ShuffleNetV2's split of kind 2: per_shuffle_ms (HOST f64[mpx_num_shuffles], may be NULL) gets every channel shuffle launch
 * of the forward. */
int mpx_profile_collect_shuffle(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                                double* per_norm_ms, double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms);
/* The same with EfficientNet-B0's split of kind 2: per_se_gate_ms / per_se_scale_ms (HOST f64[mpx_num_se] each, may be NULL) get the gate and
 * the scale launch of every SE layer. */
int mpx_profile_collect_se(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms, double* per_norm_ms,
                           double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms, double* per_se_gate_ms,
                           double* per_se_scale_ms);
/* The same with ConvNeXt's split of kind 2: per_lnorm_ms (HOST f64[mpx_num_lnorms], may be NULL) gets the launch of every stand-alone
 * LayerNorm (classifier.0's is the pooled LayerNorm launch); the depthwise + LayerNorm launches are per_dw_ms's. */
int mpx_profile_collect_ln(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms, double* per_norm_ms,
                           double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms, double* per_se_gate_ms,
                           double* per_se_scale_ms, double* per_lnorm_ms);
/* The same with a ViT's split of kind 2: per_attn_ms (HOST f64[mpx_num_attn], may be NULL) gets every attention launch, *tokens_ms (may be
 * NULL) the token assembly; the LayerNorms (encoder.ln's strided launch included) are per_lnorm_ms's. */
int mpx_profile_collect_attn(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms, double* per_norm_ms,
                             double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms, double* per_se_gate_ms,
                             double* per_se_scale_ms, double* per_lnorm_ms, double* per_attn_ms, double* tokens_ms);
/* Algorithmic FLOPs (2*MAC, convs + depthwise convs + the SE layers' two FCs + a ViT's attention products + fc) of one masked forward. */
double mpx_flops_per_forward(const mpx_engine* h);

#ifdef __cplusplus
}
#endif
#endif /* MPX_H */
