#!/usr/bin/env python3
"""Per-layer conv timing (HIP events inside the engine) for one forward batch.
usage: python tools/layer_profile.py [arch] [batch] [reps]      (arch: any name of engine.ARCH_IDS; resnext50_32x4d / resnext101_32x8d and
                                                                 regnet_x_400mf .. regnet_x_8gf add the grouped 3x3 launches as rows of
                                                                 their own, with their bytes, TB/s and MFMA TFLOP/s;
                                                                 regnet_y_800mf .. regnet_y_8gf those and the SE gate and SE scale launches
                                                                 with bytes, TB/s and their share of the forward;
                                                                 convnext_tiny / convnext_small the depthwise 7x7 + LayerNorm launches and the
                                                                 stand-alone LayerNorms, with bytes, TB/s and the shares by op class;
                                                                 vit_b_16 / vit_b_32 the attention, token assembly and LayerNorm launches
                                                                 with bytes, TB/s and the attention's MFMA TFLOP/s against its two floors)
       MPX_PER_LAYER=1 ...    one row per conv with its tile
A conv + downsample conv that run as ONE launch (K-concatenated) are booked on the main conv; they get rows of their own, with both convs'
FLOPs, under the grouped table (the grouped rows count the main conv's FLOPs only).
       MPX_TILE_SWEEP=1 ...   after the table: one row per conv with the in-network time of EVERY tile mpx_set_conv_tile accepts for it, two
                              repeats each (the spread between them is what a default may lose by)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
from network_interpretation_imagenet_amd import synth  # noqa: E402
from network_interpretation_imagenet_amd.engine import MaskedForwardEngine, MpxError  # noqa: E402

arch = sys.argv[1] if len(sys.argv) > 1 else "resnet101"
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 512
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = torch.device("cuda", 0)
eng = MaskedForwardEngine(arch, max_batch=batch, device=0).load_state_dict(synth.make_state_dict(arch))
if os.environ.get("MPX_NO_FUSION"):     # tool-only: run a stage's first conv3 and its downsample conv as two launches
    eng.set_fusion(False)
if os.environ.get("MPX_FUSION_MASK"):   # tool-only: mpx_set_fusion mask (1 = round 2's plan: no block tails; 3 = no pointwise tails)
    eng.set_fusion(int(os.environ["MPX_FUSION_MASK"]))
img = torch.from_numpy(synth.make_images(1, kind="noise")[0]).to(dev)
seg = torch.from_numpy(synth.grid_segments()).to(dev)
onoff = torch.from_numpy(synth.random_onoff(batch, 196)).to(dev)
labels = torch.zeros(batch, dtype=torch.int32, device=dev)
if os.environ.get("MPX_TILE_PATCH"):      # tool-only override: patch kernel (tile 6) wherever it is eligible
    for i, d in enumerate(eng.layers):
        try:
            eng.set_conv_tile(i, 6)
        except MpxError:
            pass
if os.environ.get("MPX_TILE_RULES"):     # tool-only: "class:tile,..." with classes k1exp k1red k1s2 k3s1 k3s2 c64k1 c64k3 stem k1x (= default tile 10 or 14)
    rules = dict(r.split(":") for r in os.environ["MPX_TILE_RULES"].split(","))
    took, kept = {}, {}
    for i, d in enumerate(eng.layers):
        if d.cin == 3:
            cls = "stem"
        elif d.cout <= 64:
            cls = "c64k1" if d.ksize == 1 else "c64k3"
        elif d.ksize == 3:
            cls = "k3s2" if d.stride == 2 else "k3s1"
        elif d.stride == 2:
            cls = "k1s2"
        else:
            cls = "k1exp" if d.cout > d.cin else "k1red"
        if "k1x" in rules and eng.conv_tile(i) in (10, 14):         # the layers whose default is the persistent expanding kernel (256->1024, 128->512)
            cls = "k1x"
        if cls in rules and d.name != b"fc":
            try:
                eng.set_conv_tile(i, int(rules[cls]))
                took[cls] = took.get(cls, 0) + 1
            except MpxError:            # the layer is not eligible for that kernel: it keeps its default -- and says so
                kept[cls] = kept.get(cls, 0) + 1
    for cls in rules:
        print("rule %s:%s -> %d layers took the tile, %d kept their default (not eligible)" % (cls, rules[cls], took.get(cls, 0), kept.get(cls, 0)))
if os.environ.get("MPX_TILE_1X1"):      # tool-only override: one tile variant on every 1x1 conv with cout >= 128
    for i, d in enumerate(eng.layers):
        if d.ksize == 1 and d.cout >= 128:
            eng.set_conv_tile(i, int(os.environ["MPX_TILE_1X1"]))
if os.environ.get("MPX_TILE_C64"):      # tool-only override: one tile variant on every cout <= 64 conv
    for i, d in enumerate(eng.layers):
        if d.cout <= 64:
            eng.set_conv_tile(i, int(os.environ["MPX_TILE_C64"]))
if os.environ.get("MPX_TILE_ALL"):      # tool-only override: force one tile variant on every conv
    for i in range(len(eng.layers)):
        eng.set_conv_tile(i, int(os.environ["MPX_TILE_ALL"]))
table = eng.stem == "table" and not os.environ.get("MPX_STEM_CONV")      # tool-only: MPX_STEM_CONV=1 = K0 + the MFMA stem (rounds 1-3)


def stage():
    if table:               # the engine's default for an image with this many rows: the stem by superposition (row 0 of the table = its apply launch)
        eng.build_stem_table(img, seg, 196)
        eng.apply_stem_table(onoff, 0)
    else:
        eng.stage_masks(img, seg, onoff, 0)


for _ in range(2):
    stage()
    eng.forward(batch, labels)
torch.cuda.synchronize()
eng.profile(True)
for _ in range(reps):
    stage()
    eng.forward(batch, labels)
eng.profile(False)
prof = eng.collect_profile()
tot = 0.0
groups = {}
# a downsample conv without a time of its own ran inside its block's last conv (K-concatenated, one launch): main conv index -> its index
names = [d.name.decode() for d in eng.layers]
fused = {}
for li, (d, ms) in enumerate(zip(eng.layers, prof["per_conv_ms"])):
    if names[li].endswith(".downsample.0") and ms == 0:
        block = names[li][:-len("downsample.0")]
        mains = [k for k, n in enumerate(names) if n in (block + "conv3", block + "conv2")]
        if mains and prof["per_conv_ms"][mains[-1]] > 0:
            fused[mains[-1]] = li
# a pointwise tail (conv3 + identity + the next block's conv1 in one launch) is booked on its conv3; its conv1 then has no time of its own
ptail_of = {c3: n1 for c3, n1 in eng.pointwise_tails() if prof["per_conv_ms"][n1] == 0}
ptail_next = {n1: c3 for c3, n1 in ptail_of.items()}


def conv_flops(li):
    """FLOPs of conv layer `li` over the batch; a grouped layer (eng.groups: 32 on a ResNeXt block's conv2) reads cin / groups channels."""
    d = eng.layers[li]
    rows = eng.conv_rows[li] or d.hout * d.hout         # a ViT's token layers run on T rows per image that are no square map (hout = 0)
    return 2.0 * batch * rows * d.cout * (d.cin // eng.groups[li]) * d.ksize * d.ksize


print("%-26s %5s %5s %2s %2s %4s %9s %9s %8s" % ("layer", "cin", "cout", "k", "s", "hout", "ms", "GFLOP", "TFLOP/s"))
for li, (d, ms) in enumerate(zip(eng.layers, prof["per_conv_ms"])):
    ms /= reps
    fl = conv_flops(li)
    key = (d.cin, d.cout, d.ksize, d.stride, d.hout)
    a = groups.setdefault(key, [0, 0.0, 0.0])
    a[0] += 1
    a[1] += ms
    a[2] += fl
    tot += ms
    if os.environ.get("MPX_PER_LAYER"):     # tool-only: one row per conv (a fused launch is booked on its main conv)
        if li in fused:     # the launch's own work: both K segments
            fl += conv_flops(fused[li])
        if li in ptail_of and ms > 0:       # the pointwise tail's own work: conv3 and the next conv1
            fl += conv_flops(ptail_of[li])
        note = ""
        if li in fused:
            note = "   + %s in the same launch (K = %d + %d)" % (names[fused[li]], d.cin * d.ksize * d.ksize, eng.layers[fused[li]].cin)
        elif li in ptail_of and ms > 0:
            note = "   + %s in the same launch (pointwise tail)" % names[ptail_of[li]]
        elif li in ptail_next and ms == 0:
            note = "   runs inside %s's launch" % names[ptail_next[li]]
        print("%-26s %5d %5d %2d %2d %4d %9.3f %9.1f %8.1f   tile %d%s" % (d.name.decode(), d.cin, d.cout, d.ksize, d.stride, d.hout, ms, fl / 1e9, fl / max(ms, 1e-9) / 1e9, eng.conv_tile(li), note))
print("-- grouped by shape --")
for key, (n, ms, fl) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
    print("%5d->%-5d k%d s%d out%-4d x%-3d %8.3f ms %5.1f%% %8.1f TFLOP/s%s" % (key[0], key[1], key[2], key[3], key[4], n, ms, 100 * ms / tot, fl / max(ms, 1e-9) / 1e9,
                                                                             "   (runs inside its block's conv3 launch)" if ms == 0 else ""))
if fused:       # the grouped rows above book these launches under their main conv's shape, with the main conv's FLOPs only
    print("-- conv + downsample conv in one launch (K-concatenated), rows of their own; GFLOP = both convs --")
    for li, lj in sorted(fused.items()):
        d, ms = eng.layers[li], prof["per_conv_ms"][li] / reps
        fl = conv_flops(li) + conv_flops(lj)
        print("%-16s + %-24s K %4d + %-4d out%-3d %8.3f ms %5.1f%% %9.1f GFLOP %8.1f TFLOP/s" % (
            names[li], names[lj], d.cin * d.ksize * d.ksize, eng.layers[lj].cin, d.hout, ms, 100 * ms / tot, fl / 1e9, fl / max(ms, 1e-9) / 1e9))
if max(eng.groups) > 1:     # ResNeXt: the grouped 3x3 launches (csrc/mpx_gconv.h, tile 16) as rows of their own, by their bytes and by their MFMA work
    print("-- grouped 3x3 convs (tile 16, RegNetX / RegNetY: csrc/mpx_gconvw.h, tile 18 -- row fragments of 16 channels per group: one launch each); bytes = split-fp16 input + output planes once; MFMA TFLOP/s = the three f16 products over "
          "channel blocks of max(cg, 16) and K padded to 32 (4x / 2x the algorithmic FLOPs at cg = 4 / 8) --")
    tot_g = g_bytes = g_fl = 0.0
    by_shape = {}
    for li, (d, ms) in enumerate(zip(eng.layers, prof["per_conv_ms"])):
        if eng.groups[li] == 1:
            continue
        ms /= reps
        cg = d.cin // eng.groups[li]
        cb = max(cg, 16)
        nbytes = batch * 4.0 * d.cin * (d.hin * d.hin + d.hout * d.hout)
        mfma_fl = 3 * 2.0 * batch * d.hout * d.hout * d.cout_pad * d.k_packed     # every row of the packed planes (= cout on a ResNeXt) x the padded K of its block, three products
        tot_g += ms
        g_bytes += nbytes
        g_fl += conv_flops(li)
        a = by_shape.setdefault((d.cin, cg, d.stride, d.hin), [0, 0.0, 0.0, 0.0, 0.0])
        a[0] += 1
        a[1] += ms
        a[2] += nbytes
        a[3] += conv_flops(li)
        a[4] += mfma_fl
        if os.environ.get("MPX_PER_LAYER"):
            print("%-18s C %4d cg %2d (block %2d, K %3d) s%d %3dx%-3d %8.3f ms %8.1f MB %6.2f TB/s %7.1f TFLOP/s algorithmic %7.1f MFMA TFLOP/s" % (
                d.name.decode(), d.cin, cg, cb, d.k_packed, d.stride, d.hin, d.hin, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9,
                conv_flops(li) / max(ms, 1e-9) / 1e9, mfma_fl / max(ms, 1e-9) / 1e9))
    for (c, cg, st, hin), (n, ms, nbytes, fl, mfl) in sorted(by_shape.items(), key=lambda kv: -kv[1][1]):
        print("C %4d cg %2d s%d %3dx%-3d x%-2d %8.3f ms %5.1f%% of the convs %9.1f MB %6.2f TB/s %7.1f TFLOP/s algorithmic %7.1f MFMA TFLOP/s" % (
            c, cg, st, hin, hin, n, ms, 100 * ms / tot, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9, fl / max(ms, 1e-9) / 1e9, mfl / max(ms, 1e-9) / 1e9))
    print("grouped convs total %.3f ms/batch = %.1f %% of the conv time (%.1f %% of their FLOPs), %.1f MB -> %.2f TB/s, %.1f TFLOP/s algorithmic"
          % (tot_g, 100 * tot_g / tot, 100 * g_fl / (eng.flops_per_forward * batch), g_bytes / 1e6, g_bytes / max(tot_g, 1e-9) / 1e9, g_fl / max(tot_g, 1e-9) / 1e9))
if eng.norms:     # DenseNet: the ops between the convs -- concat-append + BN + ReLU once per consumer of a block's concatenation, the transitions' pools
    print("-- concat-append + BN + ReLU (mpx_concat_bn_relu: one launch per stand-alone BatchNorm), grouped by map; bytes = split-fp16 read + written --")
    by_map = {}
    tot_norm = tot_bytes = 0.0
    for nd, ms in zip(eng.norms, prof["per_norm_ms"]):
        ms /= reps
        fresh = nd.channels if nd.name.endswith(b".denselayer1.norm1") else 32      # a block's first launch appends the whole block input
        nbytes = batch * nd.hw * nd.hw * 4.0 * (2 * nd.channels + fresh)        # read C, write C normalised, write the appended channels
        a = by_map.setdefault(nd.hw, [0, 0.0, 0.0, nd.channels, nd.channels])
        a[0] += 1
        a[1] += ms
        a[2] += nbytes
        a[3], a[4] = min(a[3], nd.channels), max(a[4], nd.channels)
        tot_norm += ms
        tot_bytes += nbytes
        if os.environ.get("MPX_PER_LAYER"):
            print("%-44s C %5d %3dx%-3d %9.3f ms %8.1f MB %7.2f TB/s" % (nd.name.decode(), nd.channels, nd.hw, nd.hw, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
    for hw, (n, ms, nbytes, c0, c1) in sorted(by_map.items(), reverse=True):
        print("%3dx%-3d C %4d..%-4d x%-3d %8.3f ms %9.1f MB %7.2f TB/s" % (hw, hw, c0, c1, n, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
    print("concat-append + BN + ReLU total %.3f ms/batch, %.1f MB -> %.2f TB/s; transitions' 2x2 average pools %.3f ms/batch; conv total %.3f ms/batch"
          % (tot_norm, tot_bytes / 1e6, tot_bytes / max(tot_norm, 1e-9) / 1e9, prof["avgpool2_ms"] / reps, tot))
shuffle_net = arch.startswith("shufflenet")
if eng.attns:   # ViT: the attention launches, the token assembly and the LayerNorms between the MFMA convs
    t, width = eng.attns[0].tokens, eng.attns[0].heads * eng.attns[0].head_dim
    print("-- attention (mpx_attention: one launch per encoder layer); bytes = the QKV planes read once + the output planes written once; FLOPs = Q K^T and P V --")
    tot_at = sum(prof["per_attn_ms"]) / reps
    at_bytes = batch * 4.0 * t * (3 * width + width)
    at_fl = 2.0 * batch * 2 * t * t * width
    for ad, ms in zip(eng.attns, prof["per_attn_ms"]):
        ms /= reps
        if os.environ.get("MPX_PER_LAYER"):
            print("%-34s T %3d heads %2d %9.3f ms %8.1f MB %7.2f TB/s %8.1f GFLOP %7.1f TFLOP/s" % (ad.name.decode(), ad.tokens, ad.heads, ms, at_bytes / 1e6,
                                                                                             at_bytes / max(ms, 1e-9) / 1e9, at_fl / 1e9, at_fl / max(ms, 1e-9) / 1e9))
    n_at = len(eng.attns)
    print("attention T %3d heads %2d x%-2d %9.3f ms %8.1f MB %7.2f TB/s %8.1f GFLOP %7.1f TFLOP/s (MFMA work as issued: 1.5 x -- Q K^T runs twice)"
          % (t, eng.attns[0].heads, n_at, tot_at, n_at * at_bytes / 1e6, n_at * at_bytes / max(tot_at, 1e-9) / 1e9, n_at * at_fl / 1e9, n_at * at_fl / max(tot_at, 1e-9) / 1e9))
    tok_ms = prof["tokens_ms"] / reps
    tok_bytes = batch * 4.0 * width * (2 * t - 1)
    print("token assembly                    %9.3f ms %8.1f MB %7.2f TB/s" % (tok_ms, tok_bytes / 1e6, tok_bytes / max(tok_ms, 1e-9) / 1e9))
    ln_ms = sum(prof["per_lnorm_ms"][:-1]) / reps
    ln_bytes = (len(eng.lnorms) - 1) * batch * 4.0 * width * 2 * t
    cls_ms = prof["per_lnorm_ms"][-1] / reps
    print("LayerNorm on B x T rows       x%-2d %9.3f ms %8.1f MB %7.2f TB/s; encoder.ln on the class rows %.3f ms" % (len(eng.lnorms) - 1, ln_ms, ln_bytes / 1e6, ln_bytes / max(ln_ms, 1e-9) / 1e9, cls_ms))
    gelu_ms = sum(ms for a, ms in zip(eng.epilogue_acts, prof["per_conv_ms"]) if a) / reps
    gelu_fl = sum(conv_flops(li) for li, a in enumerate(eng.epilogue_acts) if a)
    allms = sum(prof["ms"].values()) / reps
    ln_rate = ln_bytes / max(ln_ms, 1e-9) / 1e9          # TB/s the LayerNorm kernel reaches here
    conv_rate = sum(conv_flops(li) for li in range(len(eng.layers))) / max(tot, 1e-9) / 1e9     # TFLOP/s the conv kernels reach here
    print("attention against its floors, per launch: %.3f ms measured; %.3f ms for its planes at the LayerNorm kernel's %.2f TB/s; %.3f ms for its MFMA work at the conv kernels' %.1f TFLOP/s"
          % (tot_at / n_at, at_bytes / 1e9 / max(ln_rate, 1e-9), ln_rate, at_fl / 1e9 / max(conv_rate, 1e-9), conv_rate))
    print("share of the forward by op class: conv (MFMA) %.1f %% (of which the GELU convs mlp.0, tile %s, %.1f %% of the forward at %.1f TFLOP/s), attention (%d launches) %.1f %%, "
          "LayerNorms (%d) %.1f %%, token assembly %.1f %%, staging (K0) %.1f %%, head %.1f %% of %.3f ms/batch (%d launches per forward batch)"
          % (100 * tot / allms, sorted({eng.conv_tile(li) for li, a in enumerate(eng.epilogue_acts) if a}), 100 * gelu_ms / allms, gelu_fl / max(gelu_ms, 1e-9) / 1e9, n_at,
             100 * tot_at / allms, len(eng.lnorms), 100 * (ln_ms + cls_ms) / allms, 100 * tok_ms / allms, 100 * prof["ms"]["mask_apply_normalize"] / reps / allms,
             100 * prof["ms"]["head"] / reps / allms, allms, sum(prof["launches"].values()) // reps - 1))
elif eng.lnorms:  # ConvNeXt: the depthwise 7x7 + LayerNorm launches and the stand-alone LayerNorms between the MFMA convs
    print("-- depthwise 7x7 + bias + LayerNorm over C (mpx_dwconv7x7_ln: one launch per block); bytes = split-fp16 planes read once + written once: the launch's floor --")
    tot_dw = dw_bytes = tot_ln = ln_bytes = 0.0
    by_map = {}
    for dd, ms in zip(eng.dwconvs, prof["per_dw_ms"]):
        ms /= reps
        nbytes = batch * 4.0 * dd.channels * 2 * dd.hin * dd.hin
        tot_dw += ms
        dw_bytes += nbytes
        a = by_map.setdefault((dd.channels, dd.hin), [0, 0.0, 0.0])
        a[0] += 1
        a[1] += ms
        a[2] += nbytes
        if os.environ.get("MPX_PER_LAYER"):
            print("%-24s C %4d k7 %3dx%-3d %9.3f ms %8.1f MB %7.2f TB/s" % (dd.name.decode(), dd.channels, dd.hin, dd.hin, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
    for (c, hin), (n, ms, nbytes) in sorted(by_map.items()):
        print("depthwise 7x7 + LayerNorm C %4d %3dx%-3d x%-2d %9.3f ms %8.1f MB %7.2f TB/s" % (c, hin, hin, n, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
    print("-- stand-alone LayerNorms (mpx_layernorm_c; classifier.0 = mpx_global_avgpool_ln, which reads the 7x7 map and writes one row); bytes = read + written --")
    for ld, ms in zip(eng.lnorms, prof["per_lnorm_ms"]):
        ms /= reps
        pooled = ld.name == b"classifier.0"
        nbytes = batch * 4.0 * ld.channels * ((49 + 1) if pooled else 2 * ld.hw * ld.hw)
        tot_ln += ms
        ln_bytes += nbytes
        print("%-16s C %4d %3dx%-3d %9.3f ms %8.1f MB %7.2f TB/s" % (ld.name.decode(), ld.channels, 7 if pooled else ld.hw, 7 if pooled else ld.hw, ms, nbytes / 1e6,
                                                                   nbytes / max(ms, 1e-9) / 1e9))
    gelu_ms = sum(ms for a, ms in zip(eng.epilogue_acts, prof["per_conv_ms"]) if a) / reps
    gelu_fl = sum(conv_flops(li) for li, a in enumerate(eng.epilogue_acts) if a)
    allms = sum(prof["ms"].values()) / reps
    print("depthwise + LayerNorm total %.3f ms/batch, %.1f MB -> %.2f TB/s; stand-alone LayerNorms %.3f ms/batch -> %.2f TB/s; GELU convs (block.3, tile %s) %.3f ms/batch -> %.1f TFLOP/s; conv total %.3f ms/batch"
          % (tot_dw, dw_bytes / 1e6, dw_bytes / max(tot_dw, 1e-9) / 1e9, tot_ln, ln_bytes / max(tot_ln, 1e-9) / 1e9,
             sorted({eng.conv_tile(li) for li, a in enumerate(eng.epilogue_acts) if a}), gelu_ms, gelu_fl / max(gelu_ms, 1e-9) / 1e9, tot))
    print("share of the forward by op class: conv (MFMA) %.1f %% (of which the GELU convs %.1f %% of the forward), depthwise + LayerNorm (%d launches) %.1f %%, "
          "LayerNorms (%d) %.1f %%, staging (K0) %.1f %%, head %.1f %% of %.3f ms/batch (%d launches per forward batch)"
          % (100 * tot / allms, 100 * gelu_ms / allms, len(eng.dwconvs), 100 * tot_dw / allms, len(eng.lnorms), 100 * tot_ln / allms,
             100 * prof["ms"]["mask_apply_normalize"] / reps / allms, 100 * prof["ms"]["head"] / reps / allms, allms, sum(prof["launches"].values()) // reps - 1))
elif eng.ses and not eng.dwconvs:     # RegNetY: the SE gate (ReLU) and SE scale launches between a block's grouped 3x3 and its closing 1x1
    print("-- SE gate (mpx_se_gate_relu: pool + fc1 + fc2, one workgroup per image; bytes = f.b's output read once) and SE scale (mpx_se_scale, in place; bytes = the map read + written) --")
    tot_g = g_bytes = tot_s = s_bytes = 0.0
    by_shape = {}
    for se, gms, sms in zip(eng.ses, prof["per_se_gate_ms"], prof["per_se_scale_ms"]):
        gms /= reps
        sms /= reps
        gb = batch * 4.0 * se.pitch * se.hw * se.hw
        tot_g += gms
        g_bytes += gb
        tot_s += sms
        s_bytes += 2 * gb
        a = by_shape.setdefault((se.channels, se.pitch, se.q, se.hw), [0, 0.0, 0.0, 0.0])
        a[0] += 1
        a[1] += gms
        a[2] += sms
        a[3] += gb
        if os.environ.get("MPX_PER_LAYER"):
            print("%-36s C %4d pitch %4d q %3d %3dx%-3d gate %8.3f ms %8.1f MB %6.2f TB/s   scale %8.3f ms %8.1f MB %6.2f TB/s" % (
                se.name.decode(), se.channels, se.pitch, se.q, se.hw, se.hw, gms, gb / 1e6, gb / max(gms, 1e-9) / 1e9, sms, 2 * gb / 1e6, 2 * gb / max(sms, 1e-9) / 1e9))
    for (c, pitch, q, hw), (n, gms, sms, gb) in sorted(by_shape.items(), key=lambda kv: -(kv[1][1] + kv[1][2])):
        print("C %4d pitch %4d q %3d %3dx%-3d x%-2d gate %8.3f ms %8.1f MB %6.2f TB/s   scale %8.3f ms %8.1f MB %6.2f TB/s" % (
            c, pitch, q, hw, hw, n, gms, gb / 1e6, gb / max(gms, 1e-9) / 1e9, sms, 2 * gb / 1e6, 2 * gb / max(sms, 1e-9) / 1e9))
    pool_ms = prof["ms"]["pool"] / reps - tot_g - tot_s
    allms = sum(prof["ms"].values()) / reps
    print("SE gates %.3f ms/batch, %.1f MB -> %.2f TB/s; SE scales %.3f ms/batch, %.1f MB -> %.2f TB/s; global pool %.3f ms/batch; conv total %.3f ms/batch"
          % (tot_g, g_bytes / 1e6, g_bytes / max(tot_g, 1e-9) / 1e9, tot_s, s_bytes / 1e6, s_bytes / max(tot_s, 1e-9) / 1e9, pool_ms, tot))
    print("share of the forward by op class: conv (MFMA) %.1f %%, SE gate (%d launches) %.1f %%, SE scale (%d) %.1f %% -- the three extra passes over f.b's output (gate read, scale read + write) "
          "%.1f %% together --, staging (K0) %.1f %%, global pool %.1f %%, head %.1f %% of %.3f ms/batch"
          % (100 * tot / allms, len(eng.ses), 100 * tot_g / allms, len(eng.ses), 100 * tot_s / allms, 100 * (tot_g + tot_s) / allms,
             100 * prof["ms"]["mask_apply_normalize"] / reps / allms, 100 * pool_ms / allms, 100 * prof["ms"]["head"] / reps / allms, allms))
elif eng.ses:     # EfficientNet-B0: the depthwise k x k + BN + SiLU, SE gate and SE scale launches between the 1x1 convs
    print("-- depthwise k x k + BN with SiLU on load and in the epilogue (mpx_dwconv_bn_act); bytes = split-fp16 planes read + written, pitch channels per pixel --")
    tot_dw = dw_bytes = tot_g = g_bytes = tot_s = s_bytes = 0.0
    by_class = {}
    for k, (dd, ms) in enumerate(zip(eng.dwconvs, prof["per_dw_ms"])):
        ms /= reps
        ho = (dd.hin - 1) // dd.stride + 1
        nbytes = batch * 4.0 * dd.pitch * (dd.hin * dd.hin + ho * ho)
        tot_dw += ms
        dw_bytes += nbytes
        a = by_class.setdefault((eng.dw_ksizes[k], dd.stride), [0, 0.0, 0.0])
        a[0] += 1
        a[1] += ms
        a[2] += nbytes
        print("%-24s C %4d pitch %4d k%d s%d %3dx%-3d -> %3dx%-3d %9.3f ms %8.1f MB %7.2f TB/s" % (
            dd.name.decode(), dd.channels, dd.pitch, eng.dw_ksizes[k], dd.stride, dd.hin, dd.hin, ho, ho, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
    for (ks, st), (n, ms, nbytes) in sorted(by_class.items()):
        print("depthwise %dx%d stride %d x%-2d %9.3f ms %8.1f MB %7.2f TB/s" % (ks, ks, st, n, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
    print("-- SE gate (mpx_se_gate: pool + fc1 + fc2, one workgroup per image; bytes = the map read once) and SE scale (mpx_se_scale, in place; bytes = the map read + written) --")
    for se, gms, sms in zip(eng.ses, prof["per_se_gate_ms"], prof["per_se_scale_ms"]):
        gms /= reps
        sms /= reps
        gb = batch * 4.0 * se.pitch * se.hw * se.hw
        tot_g += gms
        g_bytes += gb
        tot_s += sms
        s_bytes += 2 * gb
        print("%-22s C %4d pitch %4d q %2d %3dx%-3d gate %8.3f ms %8.1f MB %6.2f TB/s   scale %8.3f ms %8.1f MB %6.2f TB/s" % (
            se.name.decode(), se.channels, se.pitch, se.q, se.hw, se.hw, gms, gb / 1e6, gb / max(gms, 1e-9) / 1e9, sms, 2 * gb / 1e6, 2 * gb / max(sms, 1e-9) / 1e9))
    pool_ms = prof["ms"]["pool"] / reps - tot_dw - tot_g - tot_s
    allms = sum(prof["ms"].values()) / reps
    print("depthwise total %.3f ms/batch, %.1f MB -> %.2f TB/s; SE gates %.3f ms/batch -> %.2f TB/s; SE scales %.3f ms/batch -> %.2f TB/s; SiLU global pool %.3f ms/batch; conv total %.3f ms/batch"
          % (tot_dw, dw_bytes / 1e6, dw_bytes / max(tot_dw, 1e-9) / 1e9, tot_g, g_bytes / max(tot_g, 1e-9) / 1e9, tot_s, s_bytes / max(tot_s, 1e-9) / 1e9, pool_ms, tot))
    print("share of the forward by op class: conv (MFMA) %.1f %%, depthwise (%d launches) %.1f %%, SE gate (%d) %.1f %%, SE scale (%d) %.1f %%, staging (K0) %.1f %%, "
          "global pool %.1f %%, head %.1f %% of %.3f ms/batch"
          % (100 * tot / allms, len(eng.dwconvs), 100 * tot_dw / allms, len(eng.ses), 100 * tot_g / allms, len(eng.ses), 100 * tot_s / allms,
             100 * prof["ms"]["mask_apply_normalize"] / reps / allms, 100 * pool_ms / allms, 100 * prof["ms"]["head"] / reps / allms, allms))
elif eng.dwconvs:   # MobileNetV2 / ShuffleNetV2: the depthwise 3x3 + BN (+ ReLU6) launches between the 1x1 convs; bytes = split-fp16 read (each input element once) + written
    print("-- depthwise 3x3 + BN%s (%s: one launch per depthwise layer); bytes = split-fp16 planes read + written, pitch channels per pixel --"
          % (("", "mpx_dwconv3x3_bn") if shuffle_net else (" + ReLU6", "mpx_dwconv3x3_bn_relu6")))
    tot_dw = tot_bytes = 0.0
    for dd, ms in zip(eng.dwconvs, prof["per_dw_ms"]):
        ms /= reps
        ho = (dd.hin - 1) // dd.stride + 1
        nbytes = batch * 4.0 * dd.pitch * (dd.hin * dd.hin + ho * ho)
        tot_dw += ms
        tot_bytes += nbytes
        print("%-22s C %4d pitch %4d s%d %3dx%-3d -> %3dx%-3d %9.3f ms %8.1f MB %7.2f TB/s" % (
            dd.name.decode(), dd.channels, dd.pitch, dd.stride, dd.hin, dd.hin, ho, ho, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
    tot_sh = 0.0
    if shuffle_net:     # the channel shuffles: bytes = the bf real channels of a and of b read + the 2 hp channels of y written, split-fp16
        import ctypes as C
        print("-- channel shuffles (mpx_shuffle2_concat: one launch per block); bytes = 2 bf channels read + 2 hp written per pixel, split-fp16 --")
        sh_bytes = 0.0
        for k, ms in enumerate(prof["per_shuffle_ms"]):
            ms /= reps
            v = [C.c_int() for _ in range(5)]
            eng._lib.mpx_shuffle_info(eng._h, k, *[C.byref(q) for q in v])
            side, bf, hp, a_pitch, b_pitch = (q.value for q in v)
            nbytes = batch * 4.0 * side * side * (2 * bf + 2 * hp)
            tot_sh += ms
            sh_bytes += nbytes
            print("shuffle %2d  bf %3d hp %3d a_pitch %4d b_pitch %4d %3dx%-3d %9.3f ms %8.1f MB %7.2f TB/s" % (
                k, bf, hp, a_pitch, b_pitch, side, side, ms, nbytes / 1e6, nbytes / max(ms, 1e-9) / 1e9))
        print("shuffles total %.3f ms/batch, %.1f MB -> %.2f TB/s" % (tot_sh, sh_bytes / 1e6, sh_bytes / max(tot_sh, 1e-9) / 1e9))
    pool_ms = prof["ms"]["pool"] / reps - tot_dw - tot_sh
    allms = sum(prof["ms"].values()) / reps
    if shuffle_net:
        print("share of the forward by op class: conv (MFMA) %.1f %%, depthwise (%d launches) %.1f %%, shuffles (%d launches) %.1f %%, staging (K0) %.1f %%, "
              "max pool + global pool %.1f %%, head %.1f %% of %.3f ms/batch (%d launches per forward batch)"
              % (100 * tot / allms, len(eng.dwconvs), 100 * tot_dw / allms, len(prof["per_shuffle_ms"]), 100 * tot_sh / allms, 100 * prof["ms"]["mask_apply_normalize"] / reps / allms,
                 100 * pool_ms / allms, 100 * prof["ms"]["head"] / reps / allms, allms, sum(prof["launches"].values()) // reps - 1))
    print("depthwise total %.3f ms/batch, %.1f MB -> %.2f TB/s; %s %.3f ms/batch; conv total %.3f ms/batch"
          % (tot_dw, tot_bytes / 1e6, tot_bytes / max(tot_dw, 1e-9) / 1e9, "max pool + global pool" if shuffle_net else "clamped global pool", pool_ms, tot))
    if not shuffle_net:
        print("share of the forward by op class: conv (MFMA) %.1f %%, depthwise %.1f %%, staging (K0) %.1f %%, global pool %.1f %%, head %.1f %%"
              % (100 * tot / allms, 100 * tot_dw / allms, 100 * prof["ms"]["mask_apply_normalize"] / reps / allms, 100 * pool_ms / allms,
                 100 * prof["ms"]["head"] / reps / allms))
if arch.startswith("squeezenet"):     # SqueezeNet: the Fire modules' convs by their bytes (they are memory-bound), and the average pool that writes the logits
    import ctypes as C
    print("-- Fire modules: split-fp16 bytes read (the input map once) + written per launch; the expand convs write their half of the concatenation --")
    tot_bytes = {"squeeze": 0.0, "expand1x1": 0.0, "expand3x3": 0.0}
    tot_ms = dict.fromkeys(tot_bytes, 0.0)
    for li, (d, ms) in enumerate(zip(eng.layers, prof["per_conv_ms"])):
        kind = d.name.decode().rsplit(".", 1)[-1]
        if kind not in tot_bytes:
            continue
        ms /= reps
        pitch, off = C.c_int(), C.c_int()
        eng._lib.mpx_conv_out_slice(eng._h, li, C.byref(pitch), C.byref(off))
        cin_p = -(-d.cin // 32) * 32
        nbytes = batch * 4.0 * d.hout * d.hout * (cin_p + (d.cout if kind != "squeeze" else pitch.value))
        tot_bytes[kind] += nbytes
        tot_ms[kind] += ms
        print("%-22s %4d->%-4d k%d %3dx%-3d pitch %4d offset %3d tile %d %8.3f ms %8.1f MB %6.2f TB/s %7.1f TFLOP/s" % (
            d.name.decode(), d.cin, d.cout, d.ksize, d.hout, d.hout, pitch.value, off.value, eng.conv_tile(li), ms, nbytes / 1e6,
            nbytes / max(ms, 1e-9) / 1e9, conv_flops(li) / max(ms, 1e-9) / 1e9))
    for kind in tot_bytes:
        print("%-10s total %8.3f ms/batch %9.1f MB -> %5.2f TB/s" % (kind, tot_ms[kind], tot_bytes[kind] / 1e6, tot_bytes[kind] / max(tot_ms[kind], 1e-9) / 1e9))
    # the average pool (mpx_global_avgpool_logits) shares the profile's 'pool' kind with the three max pools: timed here as a launch of its own
    # over planes of classifier.1's shape, through the same event pairs
    hw, c = eng.layers[-1].hout ** 2, eng.layers[-1].cout
    ph = torch.rand(batch, hw, c, device=dev).half()
    pl = (torch.rand(batch, hw, c, device=dev) * 1e-3).half()
    lg = torch.empty(batch, c, dtype=torch.float32, device=dev)
    args = (eng._h, C.c_void_p(ph.data_ptr()), C.c_void_p(pl.data_ptr()), C.c_void_p(lg.data_ptr()), batch, hw, c, c, eng._stream())
    eng._lib.mpx_global_avgpool_logits(*args)
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(reps):
        eng._lib.mpx_global_avgpool_logits(*args)
    eng.profile(False)
    avg_ms = eng.collect_profile()["ms"]["pool"] / reps
    nbytes = batch * 4.0 * (hw * c + c)
    pool_ms = prof["ms"]["pool"] / reps
    allms = sum(prof["ms"].values()) / reps
    print("average pool -> logits (mpx_global_avgpool_logits, one launch) %3dx%-3d C %d: %8.3f ms %8.1f MB %6.2f TB/s; the four pool launches in the network %.3f ms/batch"
          % (eng.layers[-1].hout, eng.layers[-1].hout, c, avg_ms, nbytes / 1e6, nbytes / max(avg_ms, 1e-9) / 1e9, pool_ms))
    print("share of the forward by op class: conv (MFMA) %.1f %%, staging (K0) %.1f %%, pools %.1f %%, head %.1f %% of %.3f ms/batch (%d launches per forward batch)"
          % (100 * tot / allms, 100 * prof["ms"]["mask_apply_normalize"] / reps / allms, 100 * pool_ms / allms, 100 * prof["ms"]["head"] / reps / allms, allms,
             sum(prof["launches"].values()) // reps - 1))
    del ph, pl, lg
if arch == "googlenet":     # GoogLeNet: the clipped 3x3 max pools as launches of their own, and each module's launches side by side
    import ctypes as C
    print("-- clipped-window 3x3 max pools (mpx_maxpool3x3_clip: one launch each); bytes = split-fp16 planes, one read of the map + one write, pitch channels per pixel --")
    pools = []
    for k in range(eng._lib.mpx_num_clip_pools(eng._h)):
        v = [C.c_int() for _ in range(4)]
        eng._lib.mpx_clip_pool_info(eng._h, k, *[C.byref(q) for q in v])
        pools.append(tuple(q.value for q in v))
    mods = [n[:-len(".branch1.conv")] for n in names if n.endswith(".branch1.conv")]
    pool_names = ["maxpool1", "maxpool2"] + [x for m in mods for x in (["maxpool3"] if m == "inception4a" else []) + [m + ".branch4.0"]]
    tot_cp = tot_bytes = s1_ms = s1_bytes = 0.0
    cp_ms = {}
    for name, (hin, stride, pad, pitch), ms in zip(pool_names, pools, prof["per_clip_pool_ms"]):
        ms /= reps
        ho = hin if stride == 1 else -(-(hin - 3) // 2) + 1
        nbytes = batch * 4.0 * pitch * (hin * hin + ho * ho)
        tot_cp += ms
        tot_bytes += nbytes
        if stride == 1:
            s1_ms += ms
            s1_bytes += nbytes
        cp_ms[name] = ms
        print("%-24s pitch %4d s%d p%d %3dx%-3d -> %3dx%-3d %9.3f ms %8.1f MB %7.2f TB/s" % (name, pitch, stride, pad, hin, hin, ho, ho, ms, nbytes / 1e6,
                                                                                            nbytes / max(ms, 1e-9) / 1e9))
    allms = sum(prof["ms"].values()) / reps
    print("clipped pools total %.3f ms/batch, %.1f MB -> %.2f TB/s (the nine stride-1 pools %.3f ms, %.2f TB/s; the three stride-2 pools %.3f ms, %.2f TB/s)"
          % (tot_cp, tot_bytes / 1e6, tot_bytes / max(tot_cp, 1e-9) / 1e9, s1_ms, s1_bytes / max(s1_ms, 1e-9) / 1e9, tot_cp - s1_ms,
             (tot_bytes - s1_bytes) / max(tot_cp - s1_ms, 1e-9) / 1e9))
    print("-- per Inception module, ms per batch: the three 1x1 convs that read the module input | the two 3x3 convs | the pool | branch4.1 --")
    per = dict(zip(names, [ms / reps for ms in prof["per_conv_ms"]]))
    heads = 0.0
    for m in mods:
        h3 = [per["%s.%s.conv" % (m, b)] for b in ("branch1", "branch2.0", "branch3.0")]
        k3 = per[m + ".branch2.1.conv"] + per[m + ".branch3.1.conv"]
        heads += sum(h3)
        print("%-12s 1x1 heads %.3f + %.3f + %.3f = %.3f | 3x3 %.3f | pool %.3f | branch4.1 %.3f | module %.3f ms" % (
            m, h3[0], h3[1], h3[2], sum(h3), k3, cp_ms[m + ".branch4.0"], per[m + ".branch4.1.conv"],
            sum(h3) + k3 + cp_ms[m + ".branch4.0"] + per[m + ".branch4.1.conv"]))
    other_pool = prof["ms"]["pool"] / reps - tot_cp
    print("share of the forward by op class: conv (MFMA) %.1f %% (of which the 27 same-input 1x1 heads %.1f %% of the forward), clipped pools %.1f %%, "
          "maxpool4 + global average pool %.1f %%, staging (K0) %.1f %%, head %.1f %% of %.3f ms/batch (%d launches per forward batch)"
          % (100 * tot / allms, 100 * heads / allms, 100 * tot_cp / allms, 100 * other_pool / allms,
             100 * prof["ms"]["mask_apply_normalize"] / reps / allms, 100 * prof["ms"]["head"] / reps / allms, allms,
             sum(prof["launches"].values()) // reps - 1))
tails = eng.bottleneck_tails()
if tails and not os.environ.get("MPX_NO_FUSION") and int(os.environ.get("MPX_FUSION_MASK", "3")) & 3 == 3:
    names = [d.name.decode() for d in eng.layers]
    print("-- block tails (one launch each: conv2 -> conv3 + identity -> next conv1; the time is booked on the conv2 row; the tail with the"
          " downsample branch runs its block's own conv1 too) --")
    for c2, c3, ds, n1 in tails:
        print("  %s%-16s + %s%s + %-16s %8.3f ms" % ((names[c2 - 1] + " + ") if ds >= 0 else "", names[c2], names[c3],
                                                      (" + " + names[ds]) if ds >= 0 else "", names[n1], prof["per_conv_ms"][c2] / reps))
if ptail_of:
    names = [d.name.decode() for d in eng.layers]
    print("-- pointwise tails (one launch each: conv3 + identity -> next conv1; the time is booked on the conv3 row) --")
    for c3, n1 in sorted(ptail_of.items()):
        fl = conv_flops(c3) + conv_flops(n1)
        ms = prof["per_conv_ms"][c3] / reps
        print("  %-16s + %-16s %8.3f ms %9.1f GFLOP %8.1f TFLOP/s" % (names[c3], names[n1], ms, fl / 1e9, fl / max(ms, 1e-9) / 1e9))
layer1 = sum(ms for d, ms in zip(eng.layers, prof["per_conv_ms"]) if d.name.startswith(b"layer1.") or d.name == b"layer2.0.conv1") / reps
if not eng.ses and not eng.lnorms:     # (a ResNet's line; an EfficientNet or ConvNeXt engine has no layer1)
    print("layer1 (+ layer2.0.conv1): %.3f ms/batch" % layer1)
allfl = eng.flops_per_forward * batch
print("conv total %.3f ms/batch -> %.1f TFLOP/s algorithmic; other kinds ms/batch: %s" % (
    tot, allfl / tot / 1e9, {k: round(v / reps, 3) for k, v in prof["ms"].items()}))

if os.environ.get("MPX_TILE_SWEEP"):     # tool-only: every eligible tile of every layer, in the network, one layer changed at a time
    def layer_ms(li):
        eng.profile(True)
        for _ in range(reps):
            stage()
            eng.forward(batch, labels)
        eng.profile(False)
        return eng.collect_profile()["per_conv_ms"][li] / reps

    print("-- every eligible tile, ms per batch in the network (two repeats); * = default --")
    for li, d in enumerate(eng.layers):
        default = eng.conv_tile(li)
        cells = []
        for t in (0, 1, 2, 4, 6, 7, 9, 10, 12, 13, 14, 16):
            try:
                eng.set_conv_tile(li, t)
            except MpxError:
                continue
            stage()
            eng.forward(batch, labels)          # warm this kernel
            cells.append("%s%d: %.3f %.3f" % ("*" if t == default else "", t, layer_ms(li), layer_ms(li)))
        eng.set_conv_tile(li, -1)
        print("%-14s %5d->%-5d k%-2d s%d out%-3d  %s" % (d.name.decode(), d.cin, d.cout, d.ksize, d.stride, d.hout, " | ".join(cells)))
