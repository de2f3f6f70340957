// mpx_plan.h -- the layer plan of every served network: host data only, no HIP call and no kernel launch.  A section of the one
// translation unit (mpx_api.hip includes it once, behind the tile table): it uses the plan structs and mpx_engine as they stand there.
#pragma once

namespace {

constexpr int kStemRun = 32;    // K elements of one kernel row of a first layer on the padded NHWC4 staging: a run of 8 pixels x 4 channels

// A dense conv as its network states it (PlanBuilder::conv).  The ten leading fields are conv_spec()'s arguments; the rest are the parts
// the families differ in, each 0 / false where a family has no such thing.
struct ConvSpec {
    std::string name, bn;       // state_dict prefixes of the conv and of its BatchNorm ("": none)
    int cin = 0, cout = 0, k = 1, stride = 1, pad = 0, hin = 1;
    int relu = 0, residual = 0;
    bool fc = false;            // the logit layer: fp32 output of logit_pitch floats per image
    bool bias = false;          // the module is Conv2d(bias=True) / a Linear: state_dict has <name>.bias (read where the layer ALSO has a BatchNorm)
    int stem_run = 0;           // > 0: the first layer, which reads the padded NHWC4 staging one run of stem_run K elements per kernel row:
                                // kStemRun (8 pixels), 64 (AlexNet's 11-wide row: 16 pixels, two K steps), 4 * k (ViT's patch row: k pixels)
    int cin_pad = 0;            // channels per input pixel; 0: cin, or cin rounded up to 32 on a PlanBuilder::pitch32 network (the stem excepted)
    int cout_store = 0;         // channels per output pixel; 0: logit_pitch (fc), else cout, rounded up to 32 on a pitch32 network
    int y_pitch = 0, y_offset = 0;  // output slice (SqueezeNet's expands, GoogLeNet's branch ends, ShuffleNetV2's stride-2 branch ends)
    int x_pitch = 0, x_offset = 0;  // input slice (ShuffleNetV2: a stride-1 block's branch2.0)
    int in_bf = 0, in_hp = 0;   // the input is a two-half stage map (ShuffleNetV2)
    int consumer_act = 0;       // SiLU taken by the one consumer on load (EfficientNet-B0)
    int epi_act = 0;            // exact GELU in the epilogue (ConvNeXt block.3, ViT mlp.0)
    int rows = 0;               // a token layer on `rows` rows per image that are no square map (ViT)
    int tile_default = -1;      // the family's own default tile, taken where the layer is eligible for it (DenseNet's conv2: the patch kernel)
    bool generic_only = false;  // the family keeps the layer on the generic tiles whatever default_tile says (ShuffleNetV2's padded planes)
    ConvSpec& stem(int run) { stem_run = run; return *this; }
    ConvSpec& logits() { fc = true; return *this; }
    ConvSpec& biased() { bias = true; return *this; }
};

ConvSpec conv_spec(const std::string& name, const std::string& bn, int cin, int cout, int k, int stride, int pad, int hin, int relu, int residual = 0) {
    ConvSpec s;
    s.name = name; s.bn = bn;
    s.cin = cin; s.cout = cout; s.k = k; s.stride = stride; s.pad = pad; s.hin = hin;
    s.relu = relu; s.residual = residual;
    return s;
}

// A depthwise layer as its network states it (PlanBuilder::dw)
struct DwSpec {
    std::string name, bn;
    int channels = 0, pitch = 0, stride = 1, hin = 0;
    int clamp_in = 0;           // reads an MFMA conv that ReLU6 follows (MobileNetV2)
    bool linear = false;        // BatchNorm only (ShuffleNetV2)
    int in_bf = 0, in_hp = 0;   // its planes are a two-half stage map (ShuffleNetV2)
    int ksize = 3;
    bool mb = false;            // EfficientNet-B0's kernel, with SiLU on load (act_in) and in the epilogue (act_out)
    int act_in = 0, act_out = 0;
    bool ln = false;            // ConvNeXt: + bias + LayerNorm over the channels
};

// The ONE place where a layer of the plan is made: every build_topology* below states its network -- widths, depths, the block loop, the
// buffer choreography -- through these members, and no ConvLayer, DwLayer, LnLayer or SeLayer field is assigned anywhere else (the
// downsample links of a pair of layers excepted: link_downsample).  Built once per mpx_create: as plain as it can be.
struct PlanBuilder {
    mpx_engine* h;
    bool pitch32 = false;       // the network stores every map with its channels rounded up to 32 (zero weight columns, zero scale and shift on the
                                // padded rows: exact zeros): the small networks, MobileNetV2, SqueezeNet, GoogLeNet, EfficientNet-B0, the RegNets

    static int pitch_of(int c) { return (int)round_up((size_t)c, kSmallCPad); }

    // default_tile's rules restricted to the generic tiles: 64-row tiles for cout <= 64, tile 0 for 3x3, tile 7 for the expanding 1x1 layers,
    // tile 2 for the reducing ones
    static int generic_tile(int cin, int cout, int k) { return cout <= 64 ? (k >= 3 ? 1 : 4) : (k == 3 ? 0 : (cout > cin ? 7 : 2)); }

    int conv(const ConvSpec& s) {
        ConvLayer L;
        std::memset(&L.d, 0, sizeof L.d);
        set_name(L.d.name, s.name);
        set_name(L.d.bn_name, s.bn);
        L.d.cin = s.cin; L.d.cout = s.cout; L.d.ksize = s.k; L.d.stride = s.stride; L.d.pad = s.pad;
        // a token layer is no square map: it reports hin = hout = 0 (mpx_conv_rows reports its rows)
        L.d.hin = s.rows ? 0 : s.hin;
        L.d.hout = s.rows ? 0 : (s.hin + 2 * s.pad - s.k) / s.stride + 1;
        L.d.relu = s.relu; L.d.residual = s.residual;
        L.is_fc = s.fc;
        L.has_bias = s.bias;
        L.is_stem = s.stem_run > 0;
        L.consumer_act = s.consumer_act; L.epi_act = s.epi_act; L.rows = s.rows;
        L.cin_pad = s.cin_pad ? s.cin_pad : (pitch32 && !L.is_stem ? pitch_of(s.cin) : s.cin);
        L.cout_store = s.cout_store ? s.cout_store : (s.fc ? h->logit_pitch : (pitch32 ? pitch_of(s.cout) : s.cout));
        L.y_pitch = s.y_pitch; L.y_offset = s.y_offset;
        L.x_pitch = s.x_pitch; L.x_offset = s.x_offset;
        L.in_bf = s.in_bf; L.in_hp = s.in_hp;
        // K of the packed planes: one run per kernel ROW for the layer on the staging (7 * 32 for the 7x7 stems of the ResNets, DenseNets
        // and GoogLeNet; 3 * 32 for VGG, MobileNetV2, SqueezeNet, ShuffleNetV2, EfficientNet-B0 and the RegNets; 4 * 32 ConvNeXt; 11 * 64
        // AlexNet; p * 4 p ViT), else every tap over the input pitch
        L.d.k_packed = L.is_stem ? s.k * s.stem_run : s.k * s.k * L.cin_pad;
        // rows of the packed planes: the stored channels where a slice stores more than cout (GoogLeNet's inception4d.branch4.1: 64 -> 80,
        // rows of zeros).  Everywhere else cout_store is at most cout rounded up to 32, and the max changes nothing: 128 is a multiple of 32
        L.d.cout_pad = (int)round_up(std::max(s.cout, L.cout_store), 128);
        L.tile = default_tile(L.d);
        // default_tile judges the descriptor alone and may hand out kernels that know no pitch, slice or activation: the layer's own default
        const TileRow* own = s.tile_default >= 0 ? find_tile(s.tile_default) : nullptr;
        const TileRow* dflt = find_tile(L.tile);
        if (own && eligible(*own, L)) L.tile = L.tile_default = s.tile_default;      // DenseNet
        else if (L.epi_act) L.tile = L.tile_default = 7;        // ConvNeXt, ViT: only the generic kernel's epilogue has GELU; tile 7 is what default_tile gives the one such shape no persistent kernel takes
        else if (L.x_pitch || L.y_pitch || s.generic_only)      // SqueezeNet, GoogLeNet, ShuffleNetV2: only the generic kernel has a SLICE form
            L.tile = L.tile_default = generic_tile(s.cin, s.cout, s.k);
        else if (!dflt || !eligible(*dflt, L)) L.tile = L.tile_default = 2;        // the RegNets' guard (no layer of any served network: default_tile hands the padded layers generic tiles only)
        h->convs.push_back(L);
        return (int)h->convs.size() - 1;
    }
    int conv(const std::string& name, const std::string& bn, int cin, int cout, int k, int stride, int pad, int hin, int relu, int residual = 0) {
        return conv(conv_spec(name, bn, cin, cout, k, stride, pad, hin, relu, residual));
    }

    // the grouped 3x3 conv2 of a ResNeXt block (mpx_gconv.h): w -> w in `groups` groups, dense planes
    int gconv(const std::string& name, const std::string& bn, int w, int groups, int stride, int hin) {
        ConvLayer L;
        std::memset(&L.d, 0, sizeof L.d);
        set_name(L.d.name, name);
        set_name(L.d.bn_name, bn);
        L.d.cin = w; L.d.cout = w; L.d.ksize = 3; L.d.stride = stride; L.d.pad = 1;
        L.d.hin = hin; L.d.hout = (hin + 2 - 3) / stride + 1;
        L.d.relu = 1; L.d.residual = 0;
        L.cin_pad = w;
        L.cout_store = w;
        L.groups = groups;
        L.d.k_packed = gconv_kp(gconv_cb(w / groups));
        L.d.cout_pad = w;
        L.tile = L.tile_default = kGconvTile;
        h->convs.push_back(L);
        return (int)h->convs.size() - 1;
    }

    // a RegNet block's f.b (mpx_gconvw.h): w -> w in w / gw groups of gw channels, planes at a pitch of w rounded up to 32
    int gconvw(const std::string& name, const std::string& bn, int w, int gw, int stride, int hin) {
        ConvLayer L;
        std::memset(&L.d, 0, sizeof L.d);
        set_name(L.d.name, name);
        set_name(L.d.bn_name, bn);
        L.d.cin = w; L.d.cout = w; L.d.ksize = 3; L.d.stride = stride; L.d.pad = 1;
        L.d.hin = hin; L.d.hout = (hin + 2 - 3) / stride + 1;
        L.d.relu = 1; L.d.residual = 0;
        L.cin_pad = pitch_of(w);
        L.cout_store = pitch_of(w);
        L.groups = w / gw;
        L.gw = true;
        L.d.k_packed = gconvw_kp(gw);
        L.d.cout_pad = L.groups * gconvw_rf(gw) * 16;
        L.tile = L.tile_default = kGconvwTile;
        h->convs.push_back(L);
        return (int)h->convs.size() - 1;
    }

    // the downsample fusion of a bottleneck block: its last 1x1 conv c3 ("main") and its downsample conv ds run as one launch (build_fused)
    void link_downsample(int c3, int ds) {
        h->convs[c3].fuse_partner = ds; h->convs[c3].fuse_main = true;
        h->convs[ds].fuse_partner = c3;
    }

    // a depthwise layer and its launch in -> out
    int dw(const DwSpec& s, int in, int out) {
        DwLayer D;
        std::memset(&D.d, 0, sizeof D.d);
        set_name(D.d.name, s.name);
        set_name(D.d.bn_name, s.bn);
        D.d.channels = s.channels; D.d.pitch = s.pitch; D.d.stride = s.stride; D.d.hin = s.hin; D.d.clamp_in = s.clamp_in;
        D.linear = s.linear;
        D.in_bf = s.in_bf; D.in_hp = s.in_hp;
        D.ksize = s.ksize; D.mb = s.mb; D.act_in = s.act_in; D.act_out = s.act_out; D.ln = s.ln;
        h->dws.push_back(D);
        op(OP_DWCONV, (int)h->dws.size() - 1, in, out, BUF_NONE, s.hin, s.pitch);
        return (int)h->dws.size() - 1;
    }

    // a stand-alone LayerNorm over c channels (hw: the map's side, 0 for token rows); its op is the caller's (OP_LNORM, OP_AVGPOOLLN, OP_LNORMROWS)
    int ln(const std::string& name, int c, int hw) {
        LnLayer N;
        std::memset(&N.d, 0, sizeof N.d);
        std::snprintf(N.d.name, sizeof N.d.name, "%s", name.c_str());
        N.d.channels = c; N.d.hw = hw;
        h->lnorms.push_back(N);
        return (int)h->lnorms.size() - 1;
    }

    // a Squeeze-and-Excitation layer on the hw x hw map in `buf`, in place: the gate launch and the scale launch
    int se(const std::string& name, int channels, int pitch, int q, int hw, bool relu, int buf) {
        SeLayer E;
        std::memset(&E.d, 0, sizeof E.d);
        std::snprintf(E.d.name, sizeof E.d.name, "%s", name.c_str());
        E.d.channels = channels; E.d.pitch = pitch; E.d.q = q; E.d.hw = hw;
        E.relu = relu;
        h->ses.push_back(E);
        h->se_pitch_max = std::max(h->se_pitch_max, pitch);
        op(OP_SEGATE, (int)h->ses.size() - 1, buf, BUF_NONE, BUF_NONE, hw, pitch);
        op(OP_SESCALE, (int)h->ses.size() - 1, buf, buf, BUF_NONE, hw, pitch);
        return (int)h->ses.size() - 1;
    }

    Op& op(int kind, int conv, int in, int out, int res, int hin, int c, int in2 = BUF_NONE) {
        h->ops.push_back(Op{kind, conv, in, out, res, hin, c, in2});
        return h->ops.back();
    }
    void conv_op(int c, int in, int out, int res = BUF_NONE, int in2 = BUF_NONE) { op(OP_CONV, c, in, out, res, 0, 0, in2); }
    void head() { op(OP_HEAD, -1, BUF_NONE, BUF_NONE, BUF_NONE, 0, 0); }

    // the first activation buffer that is not busy (entries below 0 are no buffers)
    static int pick(std::initializer_list<int> busy) {
        for (int b = 0; b < kActBufs; ++b) {
            bool used = false;
            for (int u : busy) used |= (u == b);
            if (!used) return b;
        }
        return -100;
    }
};

// The reference's small networks.  Channels are stored padded to 32 (zero weights / zero scale and
// shift on the padding, so padded channels stay exactly 0 through ReLU and residual adds).
//   MPX_ARCH_MNIST_NET: Classification_Net, generate_gp_training_data_mnist.py:86-105
//       conv1..5 = Conv2d(3x3, pad 1, BIAS) + BN + ReLU (strides 1,1,2,1,2; 1->32->32->64->64->128), conv6 = Conv2d(128,128,3,pad 1)
//       with bias and nothing else, mean over HxW, fc1 128->10.
//   MPX_ARCH_CIFAR_RESNET + depth: ResNetCifar(depth = 6n+2), models/resnet.py:77-146: conv3x3(3->16)+BN+ReLU, three stages
//       of n BasicBlocks (16, 32, 64 planes; the first block of stages 2 and 3 has stride 2 and DownsampleB = AvgPool2d(2) +
//       zero channels on the identity, :64-74), AvgPool2d(8), fc 64->10.
int build_topology_small(mpx_engine* h) {
    h->small = true;
    h->ncls = 10;
    h->logit_pitch = 16;
    PlanBuilder pb{h, true};
    int feat = 0, hlast = 0, X = 0;
    size_t act = 0;
    auto track = [&](int hout, int c) { act = std::max(act, (size_t)hout * hout * round_up(c, kSmallCPad)); };
    if (h->arch == MPX_ARCH_MNIST_NET) {
        h->img = 28; h->in_ch = 1;
        const int cfg[5][3] = {{1, 32, 1}, {32, 32, 1}, {32, 64, 2}, {64, 64, 1}, {64, 128, 2}};
        int hcur = 28, in = BUF_INPUT;
        for (int i = 0; i < 5; ++i) {
            const std::string n = "conv" + std::to_string(i + 1);
            const int c = pb.conv(conv_spec(n + ".0", n + ".1", cfg[i][0], cfg[i][1], 3, cfg[i][2], 1, hcur, 1).biased());
            const int out = (in == 0) ? 1 : 0;
            pb.conv_op(c, in, out);
            in = out;
            hcur = h->convs[c].d.hout;
            track(hcur, cfg[i][1]);
        }
        const int c6 = pb.conv(conv_spec("conv6", "", 128, 128, 3, 1, 1, hcur, 0).biased());     // bias only: packed like fc (gamma = NULL)
        X = (in == 0) ? 1 : 0;
        pb.conv_op(c6, in, X);
        feat = 128; hlast = hcur;
        h->feat = feat;
        pb.op(OP_AVGPOOL, -1, X, BUF_POOL, BUF_NONE, hlast, feat);
        pb.conv_op(pb.conv(conv_spec("fc1", "", feat, 10, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    } else {
        const int depth = h->arch - MPX_ARCH_CIFAR_RESNET;
        if (depth < 8 || (depth - 2) % 6 != 0) return MPX_E_ARG;
        const int n = (depth - 2) / 6;
        h->img = 32; h->in_ch = 3;
        int c = pb.conv("conv1", "bn1", 3, 16, 3, 1, 1, 32, 1);       // reads the 32-channel staging as any other layer: no stem run
        pb.conv_op(c, BUF_INPUT, 0);
        track(32, 16);
        X = 0;
        int inplanes = 16, hcur = 32;
        const int planes_of[3] = {16, 32, 64};
        for (int sidx = 0; sidx < 3; ++sidx) {
            const int planes = planes_of[sidx];
            for (int b = 0; b < n; ++b) {
                const int stride = (sidx > 0 && b == 0) ? 2 : 1;
                const std::string p = "layer" + std::to_string(sidx + 1) + "." + std::to_string(b) + ".";
                const int T1 = pb.pick({X});
                c = pb.conv(p + "conv1", p + "bn1", inplanes, planes, 3, stride, 1, hcur, 1);
                pb.conv_op(c, X, T1);
                const int hout = h->convs[c].d.hout;
                int res = X, T2 = -1;
                if (stride != 1 || inplanes != planes) {            // DownsampleB on the identity
                    T2 = pb.pick({X, T1});
                    pb.op(OP_AVGPAD, -1, X, T2, BUF_NONE, hcur, (int)round_up(inplanes, kSmallCPad) * 65536 + (int)round_up(planes, kSmallCPad));
                    res = T2;
                }
                const int O = pb.pick({X, T1, T2});
                c = pb.conv(p + "conv2", p + "bn2", planes, planes, 3, 1, 1, hout, 1, 1);
                pb.conv_op(c, T1, O, res);
                X = O;
                inplanes = planes;
                hcur = hout;
                track(hcur, planes);
            }
        }
        feat = 64; hlast = hcur;
        h->feat = feat;
        pb.op(OP_AVGPOOL, -1, X, BUF_POOL, BUF_NONE, hlast, feat);
        pb.conv_op(pb.conv(conv_spec("fc", "", feat, 10, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    }
    pb.head();
    h->act_elems_per_image = act;
    return 0;
}

// torchvision VGG (vgg.py: make_layers over cfgs "A" / "B" / "D" / "E", then the classifier), depth 11 / 13 / 16 / 19, with or without
// BatchNorm.  Names follow torchvision's module indices: a conv at features.i, its BatchNorm (the _bn variants) at features.(i+1), the ReLU
// after them, one index per "M" (MaxPool2d(2, 2)).  Every conv has a bias.  The classifier runs as three more layers of the conv list:
// classifier.0 = Linear(25088, 4096) as a 7x7 valid conv over the [B][7][7][512] map (torch.flatten of NCHW is channel-major, so the
// [4096][25088] weight viewed as [4096][512][7][7] is its OIHW weight), classifier.3 = Linear(4096, 4096) as a 1x1 conv, classifier.6 =
// Linear(4096, 1000), the logit layer.  AdaptiveAvgPool2d((7, 7)) on a 7x7 map and Dropout in eval are identities.  A plain chain: the
// op list ping-pongs between two activation buffers.
int build_topology_vgg(mpx_engine* h) {
    const bool bn = h->arch > MPX_ARCH_VGG_BN;
    const int depth = h->arch - (bn ? MPX_ARCH_VGG_BN : MPX_ARCH_VGG);
    constexpr int M = 0;                                    // "M" of the cfgs
    static const int cfg_a[] = {64, M, 128, M, 256, 256, M, 512, 512, M, 512, 512, M};
    static const int cfg_b[] = {64, 64, M, 128, 128, M, 256, 256, M, 512, 512, M, 512, 512, M};
    static const int cfg_d[] = {64, 64, M, 128, 128, M, 256, 256, 256, M, 512, 512, 512, M, 512, 512, 512, M};
    static const int cfg_e[] = {64, 64, M, 128, 128, M, 256, 256, 256, 256, M, 512, 512, 512, 512, M, 512, 512, 512, 512, M};
    const int* cfg = nullptr;
    int n = 0;
    switch (depth) {
        case 11: cfg = cfg_a; n = (int)(sizeof cfg_a / sizeof *cfg_a); break;
        case 13: cfg = cfg_b; n = (int)(sizeof cfg_b / sizeof *cfg_b); break;
        case 16: cfg = cfg_d; n = (int)(sizeof cfg_d / sizeof *cfg_d); break;
        case 19: cfg = cfg_e; n = (int)(sizeof cfg_e / sizeof *cfg_e); break;
        default: return MPX_E_ARG;
    }
    h->n_act_bufs = 2;
    h->act_elems_per_image = kVggActElemsPerImage;
    PlanBuilder pb{h};
    int X = BUF_INPUT, cin = 3, hcur = MPX_IMG, idx = 0;
    // every layer is a stride-1 conv with a bias, + ReLU but for the logit layer; the first one reads the staging
    auto layer = [&](const std::string& name, const std::string& bn_name, int cout, int k, int pad, bool fc = false) {
        const int O = fc ? BUF_NONE : (X == 0 ? 1 : 0);
        ConvSpec s = conv_spec(name, bn_name, cin, cout, k, 1, pad, hcur, fc ? 0 : 1).biased();
        s.fc = fc;
        if (X == BUF_INPUT) s.stem(kStemRun);
        const int c = pb.conv(s);
        pb.conv_op(c, X, O);
        cin = cout; hcur = h->convs[c].d.hout; X = O;
    };
    for (int j = 0; j < n; ++j) {
        if (cfg[j] == M) {
            const int O = X == 0 ? 1 : 0;
            pb.op(OP_MAXPOOL2, -1, X, O, BUF_NONE, hcur, cin);
            hcur /= 2;
            idx += 1;
            X = O;
        } else {
            layer("features." + std::to_string(idx), bn ? "features." + std::to_string(idx + 1) : "", cfg[j], 3, 1);
            idx += bn ? 3 : 2;
        }
    }
    // hcur = 7, cin = 512
    layer("classifier.0", "", 4096, hcur, 0);
    layer("classifier.3", "", 4096, 1, 0);
    layer("classifier.6", "", MPX_NUM_CLASSES, 1, 0, true);
    pb.head();
    return 0;
}

// torchvision AlexNet (alexnet.py): features = conv 11x11/4 pad 2 (3 -> 64), ReLU, MaxPool2d(3, 2), conv 5x5 pad 2 (64 -> 192), ReLU,
// MaxPool2d(3, 2), conv 3x3 pad 1 (192 -> 384), ReLU, conv 3x3 pad 1 (384 -> 256), ReLU, conv 3x3 pad 1 (256 -> 256), ReLU, MaxPool2d(3, 2);
// maps 224 -> 55 -> 27 -> 27 -> 13 -> 13 -> 13 -> 13 -> 6.  No BatchNorm, every layer has a bias.  The classifier runs as three more
// layers of the conv list, as VGG's: classifier.1 = Linear(9216, 4096) as a 6x6 valid conv over the [B][6][6][256] map (the [4096][9216]
// weight viewed as [4096][256][6][6] is its OIHW weight), classifier.4 = Linear(4096, 4096) as a 1x1 conv, classifier.6 = the logit layer.
// AdaptiveAvgPool2d((6, 6)) on a 6x6 map and Dropout in eval are identities.  The op list ping-pongs between two activation buffers.
int build_topology_alexnet(mpx_engine* h) {
    if (h->arch != MPX_ARCH_ALEXNET) return MPX_E_ARG;
    h->n_act_bufs = 2;
    h->act_elems_per_image = kAlexActElemsPerImage;
    PlanBuilder pb{h};
    int X = BUF_INPUT, hcur = MPX_IMG, ccur = 3;
    auto conv = [&](const char* name, int cout, int k, int stride, int pad, int relu = 1, bool fc = false) {
        const int O = fc ? BUF_NONE : (X == 0 ? 1 : 0);
        ConvSpec s = conv_spec(name, "", ccur, cout, k, stride, pad, hcur, relu).biased();
        s.fc = fc;
        if (X == BUF_INPUT) s.stem(64);     // one 16-pixel x 4-channel run (two K steps) per kernel row
        const int c = pb.conv(s);
        pb.conv_op(c, X, O);
        hcur = h->convs[c].d.hout; ccur = cout; X = O;
    };
    auto pool = [&]() {
        const int O = X == 0 ? 1 : 0;
        pb.op(OP_MAXPOOL3P0, -1, X, O, BUF_NONE, hcur, ccur);
        hcur = (hcur - 3) / 2 + 1; X = O;
    };
    conv("features.0", 64, 11, 4, 2);       // 224 -> 55
    pool();                                 // 55 -> 27
    conv("features.3", 192, 5, 1, 2);
    pool();                                 // 27 -> 13
    conv("features.6", 384, 3, 1, 1);
    conv("features.8", 256, 3, 1, 1);
    conv("features.10", 256, 3, 1, 1);
    pool();                                 // 13 -> 6
    conv("classifier.1", 4096, hcur, 1, 0); // 6x6 valid conv: K = 9216
    conv("classifier.4", 4096, 1, 1, 0);
    conv("classifier.6", MPX_NUM_CLASSES, 1, 1, 0, 0, true);
    pb.head();
    return 0;
}

// torchvision DenseNet (densenet.py; growth rate 32, bn_size 4, 64 initial features): features.conv0 (3 -> 64, 7x7 stride 2 pad 3) + norm0
// + ReLU + MaxPool2d(3, 2, 1) -- the ResNet stem shape, so the fused stem + pool launch serves it --, four dense blocks with a transition
// behind the first three, norm5 + ReLU, global average pool, classifier.  No conv has a bias.
//   dense layer j of block b on C = C_in + 32 (j - 1) channels: norm1(C) -> ReLU -> conv1 1x1 C -> 128 -> norm2 -> ReLU -> conv2 3x3 pad 1
//       128 -> 32, output concatenated behind the C input channels.  norm2 + ReLU are conv1's epilogue; conv2 has no epilogue at all.
//   transition b: norm(C) -> ReLU -> conv 1x1 C -> C / 2 -> AvgPool2d(2, 2), in torchvision's order (the conv at full resolution).
// Buffers: R = 0 the block's RAW concatenation [B][H][W][C_block], N = 1 its normalised first C channels (dense), T1 = 2 conv1's /
// the transition conv's output, T2 = 3 conv2's / the average pool's output.  One OP_CATNORM per consumer of the concatenation appends
// the fresh channels (the block input: the pooled stem / the pooled transition; then every conv2 output) to R and writes the consumer's
// relu(bn(.)) into N.
int build_topology_densenet(mpx_engine* h) {
    int blocks[4];
    switch (h->arch - MPX_ARCH_DENSENET) {
        case 121: blocks[0] = 6; blocks[1] = 12; blocks[2] = 24; blocks[3] = 16; break;
        case 169: blocks[0] = 6; blocks[1] = 12; blocks[2] = 32; blocks[3] = 32; break;
        case 201: blocks[0] = 6; blocks[1] = 12; blocks[2] = 48; blocks[3] = 32; break;
        default: return MPX_E_ARG;      // (densenet161: growth rate 48 from 96 features, C = 96 + 48 k is not a multiple of the 32-wide K step)
    }
    constexpr int G = 32, MID = 128, R = 0, N = 1, T1 = 2, T2 = 3;
    h->densenet = true;
    h->act_elems_per_image = kActElemsPerImage;
    PlanBuilder pb{h};
    auto catnorm = [&](const std::string& name, int fresh, int g, int c, int ctot, int hw) {
        NormLayer nl;
        std::memset(&nl.d, 0, sizeof nl.d);
        std::snprintf(nl.d.name, sizeof nl.d.name, "%s", name.c_str());
        nl.d.channels = c;
        nl.d.hw = hw;
        h->norms.push_back(nl);
        Op& o = pb.op(OP_CATNORM, (int)h->norms.size() - 1, fresh, N, R, hw, c);
        o.g = g; o.ctot = ctot;
    };
    int c = pb.conv(conv_spec("features.conv0", "features.norm0", 3, 64, kStemK, 2, 3, 224, 1).stem(kStemRun));
    pb.conv_op(c, BUF_INPUT, 0);
    pb.op(OP_MAXPOOL, -1, 0, BUF_STEM, BUF_NONE, 112, 64);
    int X = BUF_STEM, cin = 64, hcur = 56;
    for (int b = 0; b < 4; ++b) {
        const int ctot = cin + G * blocks[b];
        if ((size_t)hcur * hcur * ctot > kActElemsPerImage) return MPX_E_INTERNAL;
        const std::string bp = "features.denseblock" + std::to_string(b + 1) + ".denselayer";
        catnorm(bp + "1.norm1", X, cin, cin, ctot, hcur);          // the block input becomes the head of the concatenation
        for (int j = 1; j <= blocks[b]; ++j) {
            const std::string p = bp + std::to_string(j) + ".";
            c = pb.conv(p + "conv1", p + "norm2", cin, MID, 1, 1, 0, hcur, 1);
            pb.conv_op(c, N, T1);
            // conv2 (3x3, 128 -> 32) runs the patch kernel.  default_tile's rule for cout <= 64 is the 64-row tile 1, judged on the ResNets'
            // 64 -> 64 layers (where the patch kernel lost 10 %) and left as it is; here half of those rows are padding either way, and the
            // patch kernel stages the 128-channel input once per 32-channel chunk instead of once per tap.  DenseNet-121 in the network, the
            // 58 conv2 layers, ms per batch 2340 / 512: tile 1 56.1 / 13.8, tiles 0, 2, 4, 7 47.8 .. 48.7 / 11.0 .. 12.4, tile 6 30.2 / 7.5 --
            // faster on every map (56x56 30.3 -> 16.6, 28x28 16.4 -> 8.4, 14x14 8.2 -> 4.3, 7x7 1.18 -> 0.90).  A default of THIS
            // topology's layers (tile_default), not a rule of default_tile: no other network's layer can change tile.
            ConvSpec s2 = conv_spec(p + "conv2", "", MID, G, 3, 1, 1, hcur, 0);
            s2.tile_default = 6;
            c = pb.conv(s2);
            pb.conv_op(c, T1, T2);
            cin += G;
            const std::string next = j < blocks[b] ? bp + std::to_string(j + 1) + ".norm1"
                                                   : (b < 3 ? "features.transition" + std::to_string(b + 1) + ".norm" : std::string("features.norm5"));
            catnorm(next, T2, G, cin, ctot, hcur);
        }
        if (b < 3) {
            c = pb.conv("features.transition" + std::to_string(b + 1) + ".conv", "", cin, cin / 2, 1, 1, 0, hcur, 0);
            pb.conv_op(c, N, T1);
            cin /= 2;
            pb.op(OP_AVGPOOL2, -1, T1, T2, BUF_NONE, hcur, cin);
            hcur /= 2;
            X = T2;
        }
    }
    h->feat = cin;
    pb.op(OP_AVGPOOL, -1, N, BUF_POOL, BUF_NONE, hcur, cin);
    pb.conv_op(pb.conv(conv_spec("classifier", "", cin, MPX_NUM_CLASSES, 1, 1, 0, 1, 0).logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision MobileNetV2 (mobilenetv2.py, width 1.0): features.0 = conv 3 -> 32 3x3 stride 2 pad 1 + BN + ReLU6, 17 inverted-residual blocks
// (t, c, n, s) = (1,16,1,1) (6,24,2,2) (6,32,3,2) (6,64,4,2) (6,96,3,1) (6,160,3,2) (6,320,1,1), features.18 = conv 320 -> 1280 1x1 + BN +
// ReLU6, global average pool, classifier.1 = Linear(1280, 1000).  A block is 1x1 expand + BN + ReLU6 (absent when t = 1), depthwise 3x3 +
// BN + ReLU6, 1x1 project + BN without activation; with stride 1 and cin == cout the block input is added, no ReLU behind the add.  No
// conv has a bias.
// ReLU6: the MFMA convs run their ReLU epilogue and the consumer clamps at 6 as it loads (mpx_dw.h) -- every such conv is read by a
// depthwise layer (clamp_in) or by the clamped global pool (OP_AVGPOOL6).
// Channels: 16, 24 and 144 are stored with a pitch of 32, 32 and 160 (cin_pad / cout_store as the small networks: zero weight columns,
// zero scale and shift on the padded rows, so padded channels are exact zeros wherever they are read -- the next conv, the depthwise
// layer, the residual add).  Those layers are eligible for the generic tiles only (eligible()); every generic tile runs a one-step K
// loop (K = 32: the 1x1 layers on 16, 24 or 32 channels) as it is -- its prologue stages dead steps past the end of K and the last-step
// branch runs the one fragment set -- so no tile is refused and K is not padded.
// Buffers: three of 112 * 112 * 96 elements per image (features.2's expanded map): X the block input, T1 the expanded map and then --
// dead after the depthwise layer -- the block output, T2 the depthwise output.
int build_topology_mobilenet(mpx_engine* h) {
    if (h->arch != MPX_ARCH_MOBILENET + 2) return MPX_E_ARG;
    h->n_act_bufs = 3;
    h->act_elems_per_image = kMobileActElemsPerImage;
    PlanBuilder pb{h, true};
    auto add_dw = [&](const std::string& name, const std::string& bn, int c, int stride, int hin, int in, int out) {
        DwSpec d;
        d.name = name; d.bn = bn; d.channels = c; d.pitch = pb.pitch_of(c); d.stride = stride; d.hin = hin;
        d.clamp_in = 1;                     // every depthwise layer of this network reads an MFMA conv that torchvision follows with ReLU6
        pb.dw(d, in, out);
    };
    int c = pb.conv(conv_spec("features.0.0", "features.0.1", 3, 32, 3, 2, 1, MPX_IMG, 1).stem(kStemRun));    // stride 2, pad 1
    pb.conv_op(c, BUF_INPUT, 0);
    int X = 0, cin = 32, hcur = 112, idx = 1;
    static const int cfg[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2}, {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};
    for (const auto& row : cfg) {
        for (int b = 0; b < row[2]; ++b, ++idx) {
            const int t = row[0], cout = row[1], stride = b == 0 ? row[3] : 1, hidden = cin * t;
            const bool use_res = stride == 1 && cin == cout;
            const std::string p = "features." + std::to_string(idx) + ".conv.";
            const int T1 = (X + 1) % 3, T2 = (X + 2) % 3;
            if ((size_t)hcur * hcur * pb.pitch_of(hidden) > kMobileActElemsPerImage) return MPX_E_INTERNAL;
            const int hout = (hcur - 1) / stride + 1;
            if (t == 1) {
                add_dw(p + "0.0", p + "0.1", hidden, stride, hcur, X, T2);
                c = pb.conv(p + "1", p + "2", hidden, cout, 1, 1, 0, hout, 0, use_res);
            } else {
                c = pb.conv(p + "0.0", p + "0.1", cin, hidden, 1, 1, 0, hcur, 1);
                pb.conv_op(c, X, T1);
                add_dw(p + "1.0", p + "1.1", hidden, stride, hcur, T1, T2);
                c = pb.conv(p + "2", p + "3", hidden, cout, 1, 1, 0, hout, 0, use_res);
            }
            pb.conv_op(c, T2, T1, use_res ? X : BUF_NONE);
            X = T1;
            cin = cout;
            hcur = hout;
        }
    }
    const int T = (X + 1) % 3;
    c = pb.conv("features.18.0", "features.18.1", cin, 1280, 1, 1, 0, hcur, 1);
    pb.conv_op(c, X, T);
    h->feat = 1280;
    pb.op(OP_AVGPOOL6, -1, T, BUF_POOL, BUF_NONE, hcur, 1280);
    pb.conv_op(pb.conv(conv_spec("classifier.1", "", 1280, MPX_NUM_CLASSES, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision SqueezeNet 1.1 (squeezenet.py, version "1_1"): features.0 = conv 3 -> 64 3x3 stride 2 WITHOUT padding (224 -> 111) + ReLU, eight
// Fire modules features.N = Fire(cin, s, e, e) for (N, cin, s, e) = (3,64,16,64) (4,128,16,64) (6,128,32,128) (7,256,32,128) (9,256,48,192)
// (10,384,48,192) (11,384,64,256) (12,512,64,256) with a MaxPool2d(3, 2, ceil_mode=True) in front of features.3, .6 and .9, then
// classifier.1 = conv 512 -> 1000 1x1 + ReLU on the 13x13 map and a global average pool whose output is the logits (Dropout is the identity
// in eval).  A Fire module is squeeze 1x1 + ReLU, then expand1x1 and expand3x3 (pad 1) on the squeeze map, each + ReLU, concatenated along
// the channels.  Every conv has a bias and there is no BatchNorm: the layers load as the plain VGG convs do (the bias as `beta`).
// Op list, 31 launches: stem | pool 111 -> 55 | Fire 3, Fire 4 | pool 55 -> 27 | Fire 6, Fire 7 | pool 27 -> 13 | Fire 9 .. 12 | classifier.1 |
// average pool -> logits | K4b; a Fire module is three OP_CONV.
// The max pools: 111 - 3, 55 - 3 and 27 - 3 are even, so ceil((hin - 3) / 2) = floor((hin - 3) / 2) -- the ceil-mode output has the floor-mode
// size and its last window ends on the last row / column of the map, none hangs over the edge.  OP_MAXPOOL3P0 (AlexNet's unpadded
// floor-mode 3x3 stride-2 pool) therefore IS this pool; no new pool kernel.  (squeezenet1_0's 109 -> 54 -> 27 -> 13 has an odd hin - 3 at 54: not served.)
// The concatenation: expand1x1 writes channels [0, e) and expand3x3 channels [e, 2e) of the same planes [B][h][h][2e] (y_pitch / y_offset:
// the SLICE form of the generic kernel), so nothing is copied and no op joins them.
// Channels: the squeeze widths 16 and 48 are stored with a pitch of 32 and 64 (cin_pad / cout_store as MobileNetV2: zero weight columns,
// zero scale and shift on the padded rows, exact zeros in the padded channels), so K = 32 / 32 / 64 / 64 for the 1x1 expands and 288 / 288 /
// 576 / 576 for the 3x3 ones.
// Buffers: three of 111 * 111 * 64 elements per image: X the module input, S the squeeze map, Y the concatenation, which is the next X.
int build_topology_squeezenet(mpx_engine* h) {
    if (h->arch != MPX_ARCH_SQUEEZENET + 11) return MPX_E_ARG;
    h->n_act_bufs = 3;
    h->act_elems_per_image = kSqueezeActElemsPerImage;
    PlanBuilder pb{h, true};
    // every conv has a bias and a ReLU.  slice: 0 = an ordinary layer, 1 / 2 = the first / second half of a concatenation of 2 * cout channels
    auto spec = [&](const std::string& name, int cin, int cout, int k, int stride, int pad, int hin, int slice) {
        ConvSpec s = conv_spec(name, "", cin, cout, k, stride, pad, hin, 1).biased();
        if (slice) {
            s.cout_store = cout;
            s.y_pitch = 2 * cout;
            s.y_offset = slice == 2 ? cout : 0;
        }
        return s;
    };
    int c = pb.conv(spec("features.0", 3, 64, 3, 2, 0, MPX_IMG, 0).stem(kStemRun));      // stride 2, pad 0
    pb.conv_op(c, BUF_INPUT, 0);
    int X = 0, cin = 64, hcur = h->convs[c].d.hout;
    static const int fires[8][3] = {{3, 16, 64}, {4, 16, 64}, {6, 32, 128}, {7, 32, 128}, {9, 48, 192}, {10, 48, 192}, {11, 64, 256}, {12, 64, 256}};
    for (const auto& f : fires) {
        const int N = f[0], s = f[1], e = f[2];
        if (N == 3 || N == 6 || N == 9) {       // features.2 / .5 / .8
            if ((hcur - 3) % 2 != 0) return MPX_E_INTERNAL;     // ceil mode would differ from the floor-mode kernel
            const int O = (X + 1) % 3;
            pb.op(OP_MAXPOOL3P0, -1, X, O, BUF_NONE, hcur, cin);
            hcur = (hcur - 3) / 2 + 1;
            X = O;
        }
        const int S = (X + 1) % 3, Y = (X + 2) % 3;
        if ((size_t)hcur * hcur * 2 * e > kSqueezeActElemsPerImage || (size_t)hcur * hcur * pb.pitch_of(s) > kSqueezeActElemsPerImage) return MPX_E_INTERNAL;
        const std::string p = "features." + std::to_string(N) + ".";
        pb.conv_op(pb.conv(spec(p + "squeeze", cin, s, 1, 1, 0, hcur, 0)), X, S);
        pb.conv_op(pb.conv(spec(p + "expand1x1", s, e, 1, 1, 0, hcur, 1)), S, Y);
        pb.conv_op(pb.conv(spec(p + "expand3x3", s, e, 3, 1, 1, hcur, 2)), S, Y);
        X = Y;
        cin = 2 * e;
    }
    // classifier.1 is the last entry of the conv list but NOT the logit layer (is_fc): it writes split planes [B][13][13][1000] like any
    // other layer (of 1000 channels per pixel, not 1024), and the average pool behind it writes the fp32 logits
    const int T = (X + 1) % 3;
    if ((size_t)hcur * hcur * MPX_NUM_CLASSES > kSqueezeActElemsPerImage) return MPX_E_INTERNAL;
    ConvSpec sc = spec("classifier.1", cin, MPX_NUM_CLASSES, 1, 1, 0, hcur, 0);
    sc.cout_store = MPX_NUM_CLASSES;
    pb.conv_op(pb.conv(sc), X, T);
    h->feat = MPX_NUM_CLASSES;
    pb.op(OP_AVGLOGITS, -1, T, BUF_NONE, BUF_NONE, hcur, MPX_NUM_CLASSES);
    pb.head();
    return 0;
}

// torchvision GoogLeNet (googlenet.py, aux_logits off, eval mode): conv1 7x7/2 pad 3 (3 -> 64, 224 -> 112: the ResNet stem's shape, run as a
// launch of its own -- the pool behind it is not the ResNets') | maxpool1 3/2 ceil 112 -> 56 | conv2 1x1 64 -> 64 | conv3 3x3 pad 1 64 -> 192 |
// maxpool2 3/2 ceil 56 -> 28 | inception3a, 3b | maxpool3 3/2 ceil 28 -> 14 | inception4a .. 4e | maxpool4 2x2/2 ceil 14 -> 7 (exact: the VGG
// pool) | inception5a, 5b | global average pool | fc 1024 -> 1000.  Every conv is BasicConv2d = Conv2d(bias=False) + BatchNorm2d(eps 0.001) + ReLU.
// Inception(in, c1, r3, c3, r5, c5, pp) concatenates branch1 (1x1 in -> c1), branch2 (1x1 in -> r3, 3x3 pad 1 r3 -> c3), branch3 (1x1 in -> r5,
// 3x3 pad 1 r5 -> c5: torchvision's 3x3 where the paper has 5x5) and branch4 (MaxPool2d(3, 1, 1, ceil_mode=True), 1x1 in -> pp).
// Op list, 73 launches: 57 OP_CONV (the stem, conv2, conv3, six per module, fc), 12 OP_MAXPOOL3C (mpx_pool3c.h: the three stride-2 ceil-mode
// pools, whose last window hangs over the edge -- 112 - 3, 56 - 3 and 28 - 3 are odd --, and the nine stride-1 pad-1 pools), OP_MAXPOOL2,
// OP_AVGPOOL, OP_HEAD.
// THE CONCATENATION IS THE BRANCHES' EPILOGUE: branch1, branch2.1, branch3.1 and branch4.1 write channels [0, c1), [c1, c1 + c3), [c1 + c3,
// c1 + c3 + c5) and [c1 + c3 + c5, out) of one buffer (y_pitch / y_offset: the SLICE form of the generic kernel); nothing is copied.  Every
// offset is a multiple of 8.
// Channels: the reduce widths 16, 24, 48, 112 and 144 are stored with pitch 32, 32, 64, 128 and 160 (zero weight columns in the 3x3 conv that
// reads them, zero scale and shift on the padded rows: exact zeros).  inception4d's concatenation is 528 wide and feeds K = 528, not a
// multiple of the 32-wide K step: it is stored with pitch 544, and its last slice (branch4.1, 64 channels at offset 464) stores 80 -- rows
// 64 .. 79 of its weights, scale and shift are zero, so channels 528 .. 543 are WRITTEN as exact zeros by every forward.  inception4e's three
// 1x1 convs on the module input (cin_pad 544), its pool (pitch 544: the max of zeros is zero) and branch4.1 behind the pool (cin_pad 544)
// all read that pitch.
// Buffers: three of 112 * 112 * 64 elements per image (the stem's output; conv3's 56 * 56 * 192 and every concatenation are smaller): X the
// module input, T what one branch keeps between its two launches (the reduce map, the pooled input), Y the concatenation, the next X.
int build_topology_googlenet(mpx_engine* h) {
    if (h->arch != MPX_ARCH_GOOGLENET) return MPX_E_ARG;
    h->googlenet = true;
    h->n_act_bufs = 3;
    h->act_elems_per_image = kActElemsPerImage;
    PlanBuilder pb{h, true};
    // a BasicConv2d (+ ReLU).  y_pitch = 0: an ordinary layer (output pitch = cout rounded up to 32); else a slice of y_pitch-wide planes that
    // stores `store` channels
    auto spec = [&](const std::string& name, int cin, int cout, int k, int stride, int pad, int hin, int y_pitch = 0, int y_offset = 0, int store = 0) {
        ConvSpec s = conv_spec(name + ".conv", name + ".bn", cin, cout, k, stride, pad, hin, 1);
        s.y_pitch = y_pitch; s.y_offset = y_offset; s.cout_store = y_pitch ? store : 0;
        return s;
    };
    // a clipped 3x3 max pool over planes of `pitch` channels per pixel; returns the output side
    auto pool_op = [&](int in, int out, int hin, int stride, int pad, int pitch) {
        h->pools3c.push_back(ClipPool{hin, stride, pad, pitch});
        pb.op(OP_MAXPOOL3C, (int)h->pools3c.size() - 1, in, out, BUF_NONE, hin, pitch);
        return pool3c_out_side(hin, stride, pad);
    };
    pb.conv_op(pb.conv(spec("conv1", 3, 64, kStemK, 2, 3, MPX_IMG).stem(kStemRun)), BUF_INPUT, 0);
    int hcur = pool_op(0, 1, 112, 2, 0, 64);                    // maxpool1: 112 -> 56
    pb.conv_op(pb.conv(spec("conv2", 64, 64, 1, 1, 0, hcur)), 1, 2);
    pb.conv_op(pb.conv(spec("conv3", 64, 192, 3, 1, 1, hcur)), 2, 0);
    int X = 1;
    hcur = pool_op(0, X, hcur, 2, 0, 192);                      // maxpool2: 56 -> 28
    if (hcur != 28) return MPX_E_INTERNAL;
    struct Mod { const char* name; int cin, c1, r3, c3, r5, c5, pp; };
    static const Mod mods[9] = {{"inception3a", 192, 64, 96, 128, 16, 32, 32},   {"inception3b", 256, 128, 128, 192, 32, 96, 64},
                                {"inception4a", 480, 192, 96, 208, 16, 48, 64},  {"inception4b", 512, 160, 112, 224, 24, 64, 64},
                                {"inception4c", 512, 128, 128, 256, 24, 64, 64}, {"inception4d", 512, 112, 144, 288, 32, 64, 64},
                                {"inception4e", 528, 256, 160, 320, 32, 128, 128}, {"inception5a", 832, 256, 160, 320, 32, 128, 128},
                                {"inception5b", 832, 384, 192, 384, 48, 128, 128}};
    int cin = 192;
    for (int m = 0; m < 9; ++m) {
        const Mod& M = mods[m];
        if (M.cin != cin) return MPX_E_INTERNAL;
        if (m == 2 || m == 7) {
            const int O = (X + 1) % 3;
            if (m == 2) {
                hcur = pool_op(X, O, hcur, 2, 0, pb.pitch_of(cin));    // maxpool3: 28 -> 14
            } else {
                pb.op(OP_MAXPOOL2, -1, X, O, BUF_NONE, hcur, pb.pitch_of(cin));   // maxpool4: 14 -> 7, every window inside the map
                hcur /= 2;
            }
            X = O;
        }
        const int T = (X + 1) % 3, Y = (X + 2) % 3;
        const int out = M.c1 + M.c3 + M.c5 + M.pp, P = pb.pitch_of(out), Pin = pb.pitch_of(cin);
        if ((size_t)hcur * hcur * std::max(P, Pin) > kActElemsPerImage || (M.c1 | M.c3 | M.c5 | M.pp) & 7) return MPX_E_INTERNAL;
        const std::string p = std::string(M.name) + ".";
        pb.conv_op(pb.conv(spec(p + "branch1", cin, M.c1, 1, 1, 0, hcur, P, 0, M.c1)), X, Y);
        pb.conv_op(pb.conv(spec(p + "branch2.0", cin, M.r3, 1, 1, 0, hcur)), X, T);
        pb.conv_op(pb.conv(spec(p + "branch2.1", M.r3, M.c3, 3, 1, 1, hcur, P, M.c1, M.c3)), T, Y);
        pb.conv_op(pb.conv(spec(p + "branch3.0", cin, M.r5, 1, 1, 0, hcur)), X, T);
        pb.conv_op(pb.conv(spec(p + "branch3.1", M.r5, M.c5, 3, 1, 1, hcur, P, M.c1 + M.c3, M.c5)), T, Y);
        if (pool_op(X, T, hcur, 1, 1, Pin) != hcur) return MPX_E_INTERNAL;
        // the last slice also writes the concatenation's pad channels [out, P), as zeros (inception4d: 64 -> 80)
        pb.conv_op(pb.conv(spec(p + "branch4.1", cin, M.pp, 1, 1, 0, hcur, P, M.c1 + M.c3 + M.c5, M.pp + P - out)), T, Y);
        X = Y;
        cin = out;
    }
    if (cin != 1024 || hcur != 7) return MPX_E_INTERNAL;
    h->feat = cin;
    pb.op(OP_AVGPOOL, -1, X, BUF_POOL, BUF_NONE, hcur, cin);
    pb.conv_op(pb.conv(conv_spec("fc", "", cin, MPX_NUM_CLASSES, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision ShuffleNetV2 (shufflenetv2.py; x0_5 / x1_0 / x1_5 / x2_0): conv1 = Conv2d(3, 24, 3, stride 2, pad 1) + BN + ReLU (224 -> 112) |
// MaxPool2d(3, 2, 1) (112 -> 56) | stage2, stage3, stage4 of 4, 8, 4 InvertedResidual blocks on 28x28, 14x14, 7x7 maps (block 0 of a stage has
// stride 2) | conv5 = 1x1 conv to 1024 (2048 for x2_0) + BN + ReLU | mean over the 7x7 map | fc.  No conv has a bias.  With bf = oup / 2:
//   stride 1: x1, x2 = x[:, :bf], x[:, bf:];  out = cat(x1, branch2(x2))
//   stride 2: out = cat(branch1(x), branch2(x))
//   branch2 = 1x1 conv (bf -> bf on x2; stride 2: inp -> bf on x) + BN + ReLU, depthwise 3x3 (the block's stride) + BN, 1x1 conv bf -> bf + BN + ReLU
//   branch1 = depthwise 3x3 stride 2 (groups = inp) + BN, 1x1 conv inp -> bf + BN + ReLU
//   then channel_shuffle(out, 2): out'[2i] = out[i], out'[2i + 1] = out[bf + i].
// Stage maps live in the TWO-HALF layout (mpx_shuffle.h): pitch 2 hp, hp = bf rounded up to 32, the second half at hp, exact zeros on the
// pads.  A stride-1 block's branch2.0 reads the second half IN PLACE (ConvLayer::x_pitch / x_offset: the generic kernel's pix_stride is not
// its K per tap), the shuffle reads the first half in place; whoever reads a whole stage map -- the next stage's branch1.0 (depthwise),
// branch1.2, branch2.0 and conv5 -- has its weights packed at the physical channel positions (in_bf / in_hp).  conv1 and the max pool keep
// the plain layout, 24 channels at pitch 32.  The depthwise layers have no activation (DwLayer::linear: the run form without SiLU, mpx_dw.h).
// Op list, 76 launches: conv1 | OP_MAXPOOL | 13 stride-1 blocks of 4 (branch2.0, branch2.3, branch2.5, shuffle) | 3 stride-2 blocks of 6
// (branch1.0, branch1.2, branch2.0, branch2.3, branch2.5, shuffle) | conv5 | OP_AVGPOOL | fc | OP_HEAD.  38 conv entries, 19 depthwise, 16 shuffles.
// Buffers: three of 112 * 112 * 32 elements per image.  Stride 1: X the block input, T1 branch2.0's output and then branch2.5's, T2 the
// depthwise output and then the shuffled map, the next X.  Stride 2: branch1.0 X -> T1, branch1.2 T1 -> the first half of T2 (SLICE form),
// branch2.0 X -> T1, branch2.3 T1 -> X (dead from here on), branch2.5 X -> the second half of T2, the shuffle T2 -> T1, the next X.
int build_topology_shufflenet(mpx_engine* h) {
    static const int widths[4][5] = {{24, 48, 96, 192, 1024}, {24, 116, 232, 464, 1024}, {24, 176, 352, 704, 1024}, {24, 244, 488, 976, 2048}};
    const int* w = nullptr;
    switch (h->arch - MPX_ARCH_SHUFFLENET) {
        case 5: w = widths[0]; break;
        case 10: w = widths[1]; break;
        case 15: w = widths[2]; break;
        case 20: w = widths[3]; break;
        default: return MPX_E_ARG;
    }
    h->n_act_bufs = 3;
    h->act_elems_per_image = kShuffleActElemsPerImage;
    PlanBuilder pb{h};          // every pitch is stated: the two-half layout is no rounding of the channel count
    struct ConvOpt { int cin_pad, cout_store, in_bf, in_hp, x_pitch, x_offset, y_pitch, y_offset; };
    // a 1x1 conv + BN + ReLU and its launch
    auto conv1x1 = [&](const std::string& name, const std::string& bn, int cin, int cout, int hin, const ConvOpt& o, int in, int out) {
        ConvSpec s = conv_spec(name, bn, cin, cout, 1, 1, 0, hin, 1);
        s.cin_pad = o.cin_pad; s.cout_store = o.cout_store;
        s.in_bf = o.in_bf; s.in_hp = o.in_hp;
        s.x_pitch = o.x_pitch; s.x_offset = o.x_offset;
        s.y_pitch = o.y_pitch; s.y_offset = o.y_offset;
        // default_tile judges the descriptor alone; a layer that reads or writes a channel slice (PlanBuilder::conv's rule), or whose planes are
        // wider than its channels, runs the generic tiles only.  (MobileNetV2, EfficientNet-B0, GoogLeNet and the RegNets leave their padded
        // layers to default_tile, which hands them generic tiles: DESIGN.md 32)
        s.generic_only = o.cin_pad != cin;
        pb.conv_op(pb.conv(s), in, out);
    };
    auto add_dw = [&](const std::string& name, const std::string& bn, int c, int pitch, int in_bf, int in_hp, int stride, int hin, int in, int out) {
        DwSpec d;
        d.name = name; d.bn = bn; d.channels = c; d.pitch = pitch; d.stride = stride; d.hin = hin;
        d.linear = true;
        d.in_bf = in_bf; d.in_hp = in_hp;
        pb.dw(d, in, out);
    };
    auto shuffle_op = [&](int a, int b, int out, int side, int bf, int hp, int a_pitch, int b_pitch, int b_offset) {
        h->shuffles.push_back(ShuffleOp{side, bf, hp, a_pitch, b_pitch, b_offset});
        pb.op(OP_SHUFFLE, (int)h->shuffles.size() - 1, a, out, b, side, 2 * hp);
    };
    auto fits = [&](int side, int pitch) { return (size_t)side * side * pitch <= kShuffleActElemsPerImage; };
    ConvSpec s1 = conv_spec("conv1.0", "conv1.1", 3, w[0], 3, 2, 1, MPX_IMG, 1).stem(kStemRun);      // stride 2, pad 1
    s1.cout_store = pb.pitch_of(w[0]);
    pb.conv_op(pb.conv(s1), BUF_INPUT, 0);
    pb.op(OP_MAXPOOL, -1, 0, 1, BUF_NONE, 112, pb.pitch_of(w[0]));
    int X = 1, hcur = 56;
    int ibf = 0, ihp = 0, Pin = pb.pitch_of(w[0]);     // layout of the current map: plain (ihp = 0) at pitch Pin, or two halves of ibf at ihp
    static const int repeats[3] = {4, 8, 4};
    for (int s = 0; s < 3; ++s) {
        const int inp = w[s], oup = w[s + 1], bf = oup / 2, hp = pb.pitch_of(bf);
        if ((oup & 3) || (s > 0 && inp != 2 * ibf)) return MPX_E_INTERNAL;      // bf even: a shuffle unit starts on an even logical channel
        for (int b = 0; b < repeats[s]; ++b) {
            const std::string p = "stage" + std::to_string(s + 2) + "." + std::to_string(b) + ".";
            const int T1 = (X + 1) % 3, T2 = (X + 2) % 3;
            if (b == 0) {
                const int ho = (hcur - 1) / 2 + 1;
                if (!fits(hcur, Pin) || !fits(hcur, hp) || !fits(ho, 2 * hp)) return MPX_E_INTERNAL;
                add_dw(p + "branch1.0", p + "branch1.1", inp, Pin, ibf, ihp, 2, hcur, X, T1);
                conv1x1(p + "branch1.2", p + "branch1.3", inp, bf, ho, ConvOpt{Pin, hp, ibf, ihp, 0, 0, 2 * hp, 0}, T1, T2);
                conv1x1(p + "branch2.0", p + "branch2.1", inp, bf, hcur, ConvOpt{Pin, hp, ibf, ihp, 0, 0, 0, 0}, X, T1);
                add_dw(p + "branch2.3", p + "branch2.4", bf, hp, 0, 0, 2, hcur, T1, X);       // X is dead: both branches have read it
                conv1x1(p + "branch2.5", p + "branch2.6", bf, bf, ho, ConvOpt{hp, hp, 0, 0, 0, 0, 2 * hp, hp}, X, T2);
                shuffle_op(T2, T2, T1, ho, bf, hp, 2 * hp, 2 * hp, hp);
                X = T1;
                hcur = ho;
                ibf = bf; ihp = hp; Pin = 2 * hp;
            } else {
                if (!fits(hcur, 2 * hp)) return MPX_E_INTERNAL;
                conv1x1(p + "branch2.0", p + "branch2.1", bf, bf, hcur, ConvOpt{hp, hp, 0, 0, 2 * hp, hp, 0, 0}, X, T1);
                add_dw(p + "branch2.3", p + "branch2.4", bf, hp, 0, 0, 1, hcur, T1, T2);
                conv1x1(p + "branch2.5", p + "branch2.6", bf, bf, hcur, ConvOpt{hp, hp, 0, 0, 0, 0, 0, 0}, T2, T1);
                shuffle_op(X, T1, T2, hcur, bf, hp, 2 * hp, hp, 0);
                X = T2;
            }
        }
    }
    if (hcur != 7) return MPX_E_INTERNAL;
    const int T = (X + 1) % 3;
    conv1x1("conv5.0", "conv5.1", w[3], w[4], hcur, ConvOpt{Pin, w[4], ibf, ihp, 0, 0, 0, 0}, X, T);
    h->feat = w[4];
    pb.op(OP_AVGPOOL, -1, T, BUF_POOL, BUF_NONE, hcur, w[4]);
    pb.conv_op(pb.conv(conv_spec("fc", "", w[4], MPX_NUM_CLASSES, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision EfficientNet-B0 (efficientnet.py, eval mode): features.0 = conv 3 -> 32 3x3 stride 2 pad 1 + BN + SiLU, 16 MBConv blocks
// features.S.B over seven stages (t, k, s, in, out, n) = (1,3,1,32,16,1) (6,3,2,16,24,2) (6,5,2,24,40,2) (6,3,2,40,80,3) (6,5,1,80,112,3)
// (6,5,2,112,192,4) (6,3,1,192,320,1), features.8 = conv 320 -> 1280 1x1 + BN + SiLU, global average pool, classifier.1 = Linear(1280, 1000).
// A block with input cin and e = t * cin is `block` = 1x1 expand + BN + SiLU (absent when t = 1: every index below is one less), depthwise
// k x k (pad (k - 1) / 2, the block's stride) + BN + SiLU, SqueezeExcitation(e, max(1, cin / 4)) -- gate = sigmoid(fc2(silu(fc1(avgpool(x))))),
// fc1 / fc2 1x1 convs WITH bias --, 1x1 project + BN without activation; with stride 1 and cin == out the block input is added, nothing
// behind the add.  No conv but the SE's has a bias.  StochasticDepth and Dropout are the identity in eval.  BatchNorm eps 1e-5.
// SiLU: the MFMA convs run WITHOUT an activation (relu = 0) and the consumer takes silu(x) as it loads (ConvLayer::consumer_act; mpx_dw.h):
// every such conv is read by exactly one depthwise layer (act_in) or by the SiLU global pool (OP_AVGPOOLSILU).
// Channels 16, 24, 40, 80, 112, 144 and 240 are stored with a pitch of 32, 32, 64, 96, 128, 160 and 256 (zero weight columns, zero scale and
// shift: exact zeros, as MobileNetV2); those layers run the generic tiles only, and default_tile's rules give every one of them a generic tile.
// Op list, 84 launches: stem | 16 x (expand, depthwise, SE gate, SE scale in place, project) without 1.0's expand | features.8 |
// OP_AVGPOOLSILU | classifier.1 | OP_HEAD.  34 conv entries, 16 depthwise, 16 SE layers.
// Buffers: three of 112 * 112 * 96 elements per image (2.0's expanded map), as MobileNetV2: X the block input, T1 the expanded map and then
// -- dead after the depthwise layer -- the block output, T2 the depthwise output, scaled in place.  The gates: f32[max_batch][1152].
int build_topology_efficientnet(mpx_engine* h) {
    if (h->arch != MPX_ARCH_EFFICIENTNET) return MPX_E_ARG;
    h->n_act_bufs = 3;
    h->act_elems_per_image = kEffActElemsPerImage;
    PlanBuilder pb{h, true};
    // no conv has a ReLU; act: torchvision follows the conv with SiLU, which its one consumer takes on load
    auto spec = [&](const std::string& name, const std::string& bn, int cin, int cout, int hin, int act, int residual = 0) {
        ConvSpec s = conv_spec(name, bn, cin, cout, 1, 1, 0, hin, 0, residual);
        s.consumer_act = act;
        return s;
    };
    ConvSpec s0 = conv_spec("features.0.0", "features.0.1", 3, 32, 3, 2, 1, MPX_IMG, 0).stem(kStemRun);      // stride 2, pad 1
    s0.consumer_act = 1;
    pb.conv_op(pb.conv(s0), BUF_INPUT, 0);
    int X = 0, cin = 32, hcur = 112, c = 0;
    static const int cfg[7][5] = {{1, 3, 1, 16, 1}, {6, 3, 2, 24, 2}, {6, 5, 2, 40, 2}, {6, 3, 2, 80, 3}, {6, 5, 1, 112, 3}, {6, 5, 2, 192, 4}, {6, 3, 1, 320, 1}};
    for (int s = 0; s < 7; ++s) {
        for (int b = 0; b < cfg[s][4]; ++b) {
            const int t = cfg[s][0], k = cfg[s][1], stride = b == 0 ? cfg[s][2] : 1, cout = cfg[s][3], e = cin * t;
            const bool use_res = stride == 1 && cin == cout;
            const std::string p = "features." + std::to_string(s + 1) + "." + std::to_string(b) + ".block.";
            const int T1 = (X + 1) % 3, T2 = (X + 2) % 3, P = pb.pitch_of(e);
            if ((size_t)hcur * hcur * P > kEffActElemsPerImage) return MPX_E_INTERNAL;
            const int hout = (hcur - 1) / stride + 1;
            int j = 0, dw_in = X;
            if (t != 1) {
                c = pb.conv(spec(p + "0.0", p + "0.1", cin, e, hcur, 1));
                pb.conv_op(c, X, T1);
                j = 1; dw_in = T1;
            }
            const std::string js = std::to_string(j), se = p + std::to_string(j + 1), pj = p + std::to_string(j + 2);
            DwSpec d;
            d.name = p + js + ".0"; d.bn = p + js + ".1"; d.channels = e; d.pitch = P; d.stride = stride; d.hin = hcur;
            d.ksize = k; d.mb = true; d.act_in = 1; d.act_out = 1;      // every depthwise layer reads an MFMA conv that SiLU follows (1.0: the stem)
            pb.dw(d, dw_in, T2);
            pb.se(se, e, P, std::max(1, cin / 4), hout, false, T2);
            c = pb.conv(spec(pj + ".0", pj + ".1", e, cout, hout, 0, use_res));
            pb.conv_op(c, T2, T1, use_res ? X : BUF_NONE);
            X = T1;
            cin = cout;
            hcur = hout;
        }
    }
    if (hcur != 7 || cin != 320) return MPX_E_INTERNAL;
    const int T = (X + 1) % 3;
    pb.conv_op(pb.conv(spec("features.8.0", "features.8.1", cin, 1280, hcur, 1)), X, T);
    h->feat = 1280;
    pb.op(OP_AVGPOOLSILU, -1, T, BUF_POOL, BUF_NONE, hcur, 1280);
    pb.conv_op(pb.conv(conv_spec("classifier.1", "", 1280, MPX_NUM_CLASSES, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision ConvNeXt-Tiny / -Small (convnext.py, eval mode): features.0 = Conv2d(3, 96, 4, stride 4, bias) + LayerNorm2d(96), four stages
// features.1 / .3 / .5 / .7 of depths (3, 3, 9, 3) / (3, 3, 27, 3) CNBlocks of width 96, 192, 384, 768 on 56 / 28 / 14 / 7 maps, features.2 / .4 /
// .6 = LayerNorm2d(C_prev) + Conv2d(C_prev, C, 2, stride 2, bias), global average pool, classifier.0 = LayerNorm2d(768), classifier.2 =
// Linear(768, 1000).  A CNBlock is block.0 = depthwise 7x7 (pad 3, bias), block.2 = LayerNorm(C) over the channels of each pixel, block.3 =
// Linear(C, 4C) + GELU, block.5 = Linear(4C, C), output = input + layer_scale * block(input); StochasticDepth is the identity in eval.  Every
// LayerNorm has eps 1e-6.  Every channel count is a multiple of 32: no padded pitches.
// GELU: block.3's consumer is block.5, an MFMA conv, so the activation is block.3's own epilogue (ConvLayer::epi_act, ConvGelu in mpx_conv.h);
// such a layer runs the generic tiles only and defaults to tile 7, what default_tile gives the one stage (96 -> 384) whose shape no
// persistent kernel takes.  block.5 is an ordinary layer with a residual operand and the layer scale as its "BatchNorm" gamma (bn_name =
// "features.S.B.layer_scale": mean 0, var 1, eps 0, beta 0, the conv's own bias as conv_bias), on default_tile's choice.
// The stem reads the padded NHWC4 staging 3 pixels into its border, one 8-pixel run per kernel row (4 of them real): k_packed = 4 * 32.
// Op list, 65 / 119 launches: stem conv | its LayerNorm | per block (depthwise + LayerNorm, block.3, block.5) | per stage boundary
// (LayerNorm, 2x2 conv) | pool + LayerNorm | classifier.2 | OP_HEAD.  41 / 77 conv entries, 18 / 36 depthwise layers, 5 LayerNorms.
// Buffers: three of 56 * 56 * 384 elements per image (block.3's output in stage 0): X the block input and residual, T1 the LayerNorm
// output and then -- dead after block.3 -- the block output, T2 the hidden map.
int build_topology_convnext(mpx_engine* h) {
    int depths[4] = {3, 3, 9, 3};
    if (h->arch == MPX_ARCH_CONVNEXT + 2) depths[2] = 27;
    else if (h->arch != MPX_ARCH_CONVNEXT + 1) return MPX_E_ARG;
    static const int dims[4] = {96, 192, 384, 768};
    h->n_act_bufs = 3;
    h->act_elems_per_image = kCnextActElemsPerImage;
    PlanBuilder pb{h};
    // every conv is unpadded, has a bias and no ReLU; act: GELU in the epilogue
    auto spec = [&](const std::string& name, const std::string& bn, int cin, int cout, int k, int stride, int hin, int residual = 0, int act = 0) {
        ConvSpec s = conv_spec(name, bn, cin, cout, k, stride, 0, hin, 0, residual).biased();
        s.epi_act = act;
        return s;
    };
    pb.conv_op(pb.conv(spec("features.0.0", "", 3, dims[0], 4, 4, MPX_IMG).stem(kStemRun)), BUF_INPUT, 0);     // stride 4, pad 0
    int hcur = 56, c = 0;
    pb.op(OP_LNORM, pb.ln("features.0.1", dims[0], hcur), 0, 1, BUF_NONE, hcur, dims[0]);
    int X = 1;
    for (int s = 0; s < 4; ++s) {
        const int C = dims[s];
        if (s > 0) {
            const int T1 = (X + 1) % 3, T2 = (X + 2) % 3, cp = dims[s - 1];
            const std::string p = "features." + std::to_string(2 * s) + ".";
            pb.op(OP_LNORM, pb.ln(p + "0", cp, hcur), X, T1, BUF_NONE, hcur, cp);
            pb.conv_op(pb.conv(spec(p + "1", "", cp, C, 2, 2, hcur)), T1, T2);
            X = T2;
            hcur /= 2;
        }
        if ((size_t)hcur * hcur * 4 * C > kCnextActElemsPerImage) return MPX_E_INTERNAL;
        for (int b = 0; b < depths[s]; ++b) {
            const std::string p = "features." + std::to_string(2 * s + 1) + "." + std::to_string(b) + ".";
            const int T1 = (X + 1) % 3, T2 = (X + 2) % 3;
            DwSpec d;
            d.name = p + "block.0"; d.bn = p + "block.2"; d.channels = C; d.pitch = C; d.stride = 1; d.hin = hcur;
            d.ksize = CN_DW_K; d.ln = true;
            pb.dw(d, X, T1);
            c = pb.conv(spec(p + "block.3", "", C, 4 * C, 1, 1, hcur, 0, 1));
            pb.conv_op(c, T1, T2);
            c = pb.conv(spec(p + "block.5", p + "layer_scale", 4 * C, C, 1, 1, hcur, 1));
            pb.conv_op(c, T2, T1, X);          // T1 is dead after block.3
            X = T1;
        }
    }
    if (hcur != 7) return MPX_E_INTERNAL;
    h->feat = dims[3];
    pb.op(OP_AVGPOOLLN, pb.ln("classifier.0", dims[3], 1), X, BUF_POOL, BUF_NONE, hcur, dims[3]);
    pb.conv_op(pb.conv(spec("classifier.2", "", dims[3], MPX_NUM_CLASSES, 1, 1, 1).logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision vit_b_16 / vit_b_32 (vision_transformer.py, eval mode, dropout 0): conv_proj = Conv2d(3, 768, p, stride p, bias), the class
// token in front of the 14 x 14 / 7 x 7 patch rows, + encoder.pos_embedding, 12 EncoderBlocks of width 768 (ln_1, MultiheadAttention with 12
// heads of 64, residual, ln_2, Linear(768, 3072) + GELU, Linear(3072, 768), residual), encoder.ln, heads.head = Linear(768, 1000) on the
// class-token row.  Every LayerNorm has eps 1e-6.  Every Linear is a 1x1 entry of the conv list whose rows are the B * T tokens: T = 197 /
// 50 rows per image are no square map, so such a layer reports hin = hout = 0, mpx_conv_rows reports T and conv_params hands the kernels
// hin = ho = T, win = wo = 1 (ConvLayer::rows).  default_tile sees the descriptor as always: in_proj runs tile 10, out_proj and mlp.3 (residual
// operand) tile 9, mlp.0 (GELU in the epilogue, ConvGelu) the generic tile 7, heads.head tile 7, the stem tile 2.
// The stem reads the padded NHWC4 staging 3 pixels into its border, one p-pixel x 4-channel run per kernel row: k_per_tap = 4 p (64: AlexNet's
// two-step form; 128: four steps), k_packed = p * 4 p.  Rows and columns reach staging index 3 + 14 * 16 - 1 = 3 + 7 * 32 - 1 = 226 < 230.
// Descriptor names drop the leading "encoder.layers." (name[48] cannot hold "encoder.layers.encoder_layer_11.self_attention.out_proj"); the
// loader puts it back.  A bias-only layer has no bn_name: scale = 2^-e, shift = bias, what gamma 1, beta 0, mean 0, var 1, eps 0 pack to.
// Op list, 2 + 7 * 12 + 3 = 89 launches: conv_proj | token assembly | per layer (ln_1, in_proj, attention, out_proj + residual, ln_2, mlp.0 +
// GELU, mlp.3 + residual) | encoder.ln on the class rows | heads.head | OP_HEAD.  50 conv entries, 25 LayerNorms, 12 attention launches.
// Buffers, each of its own size: 0 = X [T][768] the residual stream, 1 = T1 [T][768] the patch planes, then a LayerNorm's output and the
// attention's, 2 = QKV [T][2304] in_proj's output and then -- dead behind the attention -- out_proj's, 3 = H [T][3072] the hidden rows.
int build_topology_vit(mpx_engine* h) {
    const int patch = h->arch - MPX_ARCH_VIT;
    if (patch != 16 && patch != 32) return MPX_E_ARG;
    const int side = MPX_IMG / patch, T = side * side + 1, D = kVitWidth;
    h->vit = true;
    h->vit_T = T; h->vit_D = D;
    h->n_act_bufs = 4;
    h->act_elems_buf[0] = (size_t)T * D; h->act_elems_buf[1] = (size_t)T * D;
    h->act_elems_buf[2] = (size_t)T * 3 * D; h->act_elems_buf[3] = (size_t)T * kVitMlp;
    h->act_elems_per_image = h->act_elems_buf[3];
    PlanBuilder pb{h};
    // a Linear over the T token rows of every image: a 1x1 layer with a bias and no ReLU; act: GELU in the epilogue
    auto linear = [&](const std::string& name, int cin, int cout, int residual = 0, int act = 0) {
        ConvSpec s = conv_spec(name, "", cin, cout, 1, 1, 0, 0, 0, residual).biased();
        s.rows = T; s.epi_act = act;
        return pb.conv(s);
    };
    const int X = 0, T1 = 1, QKV = 2, H = 3;
    // conv_proj reads the staging one p-pixel x 4-channel run per kernel row (stride p, pad 0): hout = side
    pb.conv_op(pb.conv(conv_spec("conv_proj", "", 3, D, patch, patch, 0, MPX_IMG, 0).biased().stem(4 * patch)), BUF_INPUT, T1);
    pb.op(OP_TOKENS, -1, T1, X, BUF_NONE, T, D);
    for (int l = 0; l < kVitLayers; ++l) {
        const std::string p = "encoder_layer_" + std::to_string(l) + ".";
        pb.op(OP_LNORM, pb.ln(p + "ln_1", D, 0), X, T1, BUF_NONE, T, D);
        pb.conv_op(linear(p + "self_attention.in_proj", D, 3 * D), T1, QKV);
        AttnLayer A;
        std::memset(&A.d, 0, sizeof A.d);
        set_name(A.d.name, p + "self_attention");
        A.d.tokens = T; A.d.heads = kVitHeads; A.d.head_dim = AT_HD;
        h->attns.push_back(A);
        pb.op(OP_ATTN, (int)h->attns.size() - 1, QKV, T1, BUF_NONE, T, D);
        pb.conv_op(linear(p + "self_attention.out_proj", D, D, 1), T1, QKV, X);      // QKV is dead behind the attention
        pb.op(OP_LNORM, pb.ln(p + "ln_2", D, 0), QKV, T1, BUF_NONE, T, D);
        pb.conv_op(linear(p + "mlp.0", D, kVitMlp, 0, 1), T1, H);
        pb.conv_op(linear(p + "mlp.3", kVitMlp, D, 1), H, X, QKV);
    }
    if (kVitHeads * AT_HD != D) return MPX_E_INTERNAL;
    h->feat = D;
    pb.op(OP_LNORMROWS, pb.ln("encoder.ln", D, 0), X, BUF_POOL, BUF_NONE, T, D);
    pb.conv_op(pb.conv(conv_spec("heads.head", "", D, MPX_NUM_CLASSES, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision RegNetX (regnet.py; BlockParams.from_init_params quantises the widths to 8 and makes each divisible by min(group width, width)):
//   name             id     stage widths          depths        group width   groups per stage
//   regnet_x_400mf   14004  32, 64, 160, 400      1, 2, 7, 12   16            2, 4, 10, 25
//   regnet_x_800mf   14008  64, 128, 288, 672     1, 3, 7, 5    16            4, 8, 18, 42
//   regnet_x_1_6gf   14016  72, 168, 408, 912     2, 4, 10, 2   24            3, 7, 17, 38
//   regnet_x_3_2gf   14032  96, 192, 432, 1008    2, 6, 15, 2   48            2, 4, 9, 21
//   regnet_x_8gf     14080  80, 240, 720, 1920    2, 5, 15, 1   120           1 (80 channels: a dense 3x3), 2, 6, 16
// stem.0 = conv 3 -> 32 3x3 stride 2 pad 1 + BN (stem.1) + ReLU, no max pool (MobileNetV2's features.0.0: the row-run form on the padded NHWC4
// staging).  trunk_output.block{s}.block{s}-{j} is a bottleneck of ratio 1: f.a 1x1 w_in -> w + BN + ReLU at the input resolution, f.b 3x3
// w -> w with w / gw groups (stride 2 in block 0 of every stage) + BN + ReLU, f.c 1x1 w -> w + BN, out = ReLU(shortcut + f.c); the shortcut is
// proj (1x1 stride 2 + BN) in block 0 of every stage and the identity elsewhere.  Global average pool, fc.  No conv has a bias.
// Channels: every plane has a pitch of round_up(width, 32) (cin_pad / cout_store as MobileNetV2: zero weight columns, zero scale and shift
// on the padded rows); the grouped kernel writes its pad channels as +0 itself (mpx_gconvw.h).  Such layers run the generic tiles (eligible()).
// Launches: one per conv -- proj is a launch of its own in every stage (the K-concatenated dual form reads planes whose pitch is their cin).
// Buffers: four, sized by the largest map of the network (f.a of block 0 runs at the previous stage's resolution): X the block input, T1
// f.a's output and then -- dead after f.b -- the block output, T2 f.b's output, T3 proj's output.
//
// torchvision RegNetY 800MF .. 8GF: the same trunk with f.se = SqueezeExcitation(w, q) between f.b and f.c in EVERY block, q = round(0.25 w_in)
// of the BLOCK's input width (32 for block1-0, the previous stage's width for the other stage openers): fc1 / fc2 are 1x1 convs with bias, ReLU
// behind fc1, sigmoid behind fc2, f.b's output times the gate.  Two launches per block on T2, in place (se_gate_kernel<true>, se_scale_kernel).
//   name             id     stage widths          depths        group width   groups per stage
//   regnet_y_800mf   15008  64, 144, 320, 784     1, 3, 8, 2    16            4, 9, 20, 49
//   regnet_y_1_6gf   15016  48, 120, 336, 888     2, 6, 17, 2   24            2, 5, 14, 37
//   regnet_y_3_2gf   15032  72, 216, 576, 1512    2, 5, 13, 1   24            3, 9, 24, 63
//   regnet_y_8gf     15080  224, 448, 896, 2016   2, 4, 10, 1   56            4, 8, 16, 36
// (regnet_y_400mf has a group width of 8, below the grouped kernel's 16; regnet_y_16gf / _32gf have 112 / 232: 7 / 15 row fragments, no whole
// number of 4-fragment chunks.  Not served.)
int build_topology_regnet(mpx_engine* h) {
    struct Row { int id; int widths[4]; int depths[4]; int gw; };
    static const Row rows[] = {
        {MPX_ARCH_REGNET + 4, {32, 64, 160, 400}, {1, 2, 7, 12}, 16},
        {MPX_ARCH_REGNET + 8, {64, 128, 288, 672}, {1, 3, 7, 5}, 16},
        {MPX_ARCH_REGNET + 16, {72, 168, 408, 912}, {2, 4, 10, 2}, 24},
        {MPX_ARCH_REGNET + 32, {96, 192, 432, 1008}, {2, 6, 15, 2}, 48},
        {MPX_ARCH_REGNET + 80, {80, 240, 720, 1920}, {2, 5, 15, 1}, 120},
        {MPX_ARCH_REGNET_Y + 8, {64, 144, 320, 784}, {1, 3, 8, 2}, 16},
        {MPX_ARCH_REGNET_Y + 16, {48, 120, 336, 888}, {2, 6, 17, 2}, 24},
        {MPX_ARCH_REGNET_Y + 32, {72, 216, 576, 1512}, {2, 5, 13, 1}, 24},
        {MPX_ARCH_REGNET_Y + 80, {224, 448, 896, 2016}, {2, 4, 10, 1}, 56},
    };
    const Row* R = nullptr;
    for (const Row& r : rows)
        if (r.id == h->arch) R = &r;
    if (!R) return MPX_E_ARG;
    h->regnet_y = h->arch >= MPX_ARCH_REGNET_Y;
    PlanBuilder pb{h, true};
    int c = pb.conv(conv_spec("stem.0", "stem.1", 3, 32, 3, 2, 1, MPX_IMG, 1).stem(kStemRun));      // stride 2, pad 1
    pb.conv_op(c, BUF_INPUT, 0);
    int X = 0, cin = 32, hcur = 112;
    for (int s = 0; s < 4; ++s) {
        const int w = R->widths[s], gw = std::min(R->gw, w);
        if (w % gw || w % 8) return MPX_E_INTERNAL;
        for (int j = 0; j < R->depths[s]; ++j) {
            const int stride = j == 0 ? 2 : 1, hout = (hcur - 1) / stride + 1;
            const std::string p = "trunk_output.block" + std::to_string(s + 1) + ".block" + std::to_string(s + 1) + "-" + std::to_string(j) + ".";
            const int T1 = (X + 1) % 4, T2 = (X + 2) % 4, T3 = (X + 3) % 4;
            int res = X;
            if (j == 0) {
                c = pb.conv(p + "proj.0", p + "proj.1", cin, w, 1, 2, 0, hcur, 0);
                pb.conv_op(c, X, T3);
                res = T3;
            }
            c = pb.conv(p + "f.a.0", p + "f.a.1", cin, w, 1, 1, 0, hcur, 1);
            pb.conv_op(c, X, T1);
            c = w / gw > 1 ? pb.gconvw(p + "f.b.0", p + "f.b.1", w, gw, stride, hcur) : pb.conv(p + "f.b.0", p + "f.b.1", w, w, 3, stride, 1, hcur, 1);
            pb.conv_op(c, T1, T2);
            if (h->regnet_y) pb.se(p + "f.se", w, pb.pitch_of(w), (int)std::lround(0.25 * cin), hout, true, T2);      // f.se on f.b's output, in place
            c = pb.conv(p + "f.c.0", p + "f.c.1", w, w, 1, 1, 0, hout, 1, 1);
            pb.conv_op(c, T2, T1, res);        // T1 is dead after f.b
            X = T1;
            cin = w;
            hcur = hout;
        }
    }
    // four buffers, sized by the largest map any layer writes (f.a of block 0 runs at the previous stage's resolution)
    size_t act_max = 0;
    for (const ConvLayer& L : h->convs) act_max = std::max(act_max, (size_t)L.d.hout * L.d.hout * L.cout_store);
    h->n_act_bufs = 4;
    h->act_elems_per_image = act_max;
    h->feat = cin;
    pb.op(OP_AVGPOOL, -1, X, BUF_POOL, BUF_NONE, hcur, pb.pitch_of(cin));
    pb.conv_op(pb.conv(conv_spec("fc", "", cin, MPX_NUM_CLASSES, 1, 1, 0, 1, 0).biased().logits()), BUF_POOL, BUF_NONE);
    pb.head();
    return 0;
}

// torchvision ResNet topology (models/resnet.py, un-vendored): conv list and op list.
int build_topology(mpx_engine* h) {
    if (h->arch == MPX_ARCH_MNIST_NET || (h->arch > MPX_ARCH_CIFAR_RESNET && h->arch < MPX_ARCH_CIFAR_RESNET + 1000))
        return build_topology_small(h);
    if (h->arch > MPX_ARCH_VGG && h->arch < MPX_ARCH_VGG_BN + 100) return build_topology_vgg(h);
    if (h->arch >= MPX_ARCH_ALEXNET && h->arch < MPX_ARCH_ALEXNET + 100) return build_topology_alexnet(h);
    if (h->arch >= MPX_ARCH_DENSENET && h->arch < MPX_ARCH_DENSENET + 1000) return build_topology_densenet(h);
    if (h->arch >= MPX_ARCH_MOBILENET && h->arch < MPX_ARCH_MOBILENET + 1000) return build_topology_mobilenet(h);
    if (h->arch >= MPX_ARCH_SQUEEZENET && h->arch < MPX_ARCH_SQUEEZENET + 1000) return build_topology_squeezenet(h);
    if (h->arch >= MPX_ARCH_GOOGLENET && h->arch < MPX_ARCH_GOOGLENET + 1000) return build_topology_googlenet(h);
    if (h->arch >= MPX_ARCH_SHUFFLENET && h->arch < MPX_ARCH_SHUFFLENET + 1000) return build_topology_shufflenet(h);
    if (h->arch >= MPX_ARCH_EFFICIENTNET && h->arch < MPX_ARCH_EFFICIENTNET + 1000) return build_topology_efficientnet(h);
    if (h->arch >= MPX_ARCH_CONVNEXT && h->arch < MPX_ARCH_CONVNEXT + 1000) return build_topology_convnext(h);
    if (h->arch >= MPX_ARCH_VIT && h->arch < MPX_ARCH_VIT + 1000) return build_topology_vit(h);
    if (h->arch >= MPX_ARCH_REGNET && h->arch < MPX_ARCH_REGNET_Y + 1000) return build_topology_regnet(h);
    h->act_elems_per_image = kActElemsPerImage;
    int depths[4];
    // ResNeXt (torchvision's Bottleneck with groups = 32): width = planes * width_per_group / 64 * groups; conv2 is the one grouped layer
    int groups = 1, wpg = 64;
    switch (h->arch) {
        case MPX_ARCH_RESNEXT + 50: depths[0] = 3; depths[1] = 4; depths[2] = 6; depths[3] = 3; h->bottleneck = true; groups = 32; wpg = 4; break;
        case MPX_ARCH_RESNEXT + 101:
            depths[0] = 3; depths[1] = 4; depths[2] = 23; depths[3] = 3; h->bottleneck = true; groups = 32; wpg = 8;
            h->act_elems_per_image = 2 * kActElemsPerImage;     // layer2.0.conv1 writes 56 * 56 * 512
            break;
        case 18: depths[0] = 2; depths[1] = 2; depths[2] = 2; depths[3] = 2; h->bottleneck = false; break;
        case 34: depths[0] = 3; depths[1] = 4; depths[2] = 6; depths[3] = 3; h->bottleneck = false; break;
        case 50: depths[0] = 3; depths[1] = 4; depths[2] = 6; depths[3] = 3; h->bottleneck = true; break;
        case 101: depths[0] = 3; depths[1] = 4; depths[2] = 23; depths[3] = 3; h->bottleneck = true; break;
        case 152: depths[0] = 3; depths[1] = 8; depths[2] = 36; depths[3] = 3; h->bottleneck = true; break;
        default: return MPX_E_ARG;
    }
    const int exp = h->bottleneck ? 4 : 1;
    // (a ResNeXt engine hands the persistent kernels -- tiles 9, 10, 13, 14 and the dual form of 13 -- dense shapes that no served ResNet
    // has: DESIGN.md 21 goes through every (shape, default tile) pair; none needed a default of its own)
    PlanBuilder pb{h};
    auto pick = PlanBuilder::pick;

    int c = pb.conv(conv_spec("conv1", "bn1", 3, 64, kStemK, 2, 3, 224, 1).stem(kStemRun));
    pb.conv_op(c, BUF_INPUT, 0);
    pb.op(OP_MAXPOOL, -1, 0, BUF_STEM, BUF_NONE, 112, 64);      // the pooled planes have a buffer of their own: nothing overwrites them
    int X = BUF_STEM, cin = 64, hcur = 56;
    const int planes[4] = {64, 128, 256, 512};
    struct BlockRec { int c1, c2, c3, ds, hin; };
    std::vector<BlockRec> blocks;       // bottleneck blocks in forward order (the block-tail plan below is built from them)
    for (int s = 0; s < 4; ++s) {
        const int pl = planes[s];                   // the block's output is pl * exp channels
        const int w = pl * wpg / 64 * groups;       // its inner width (= pl on a ResNet)
        for (int b = 0; b < depths[s]; ++b) {
            const int stride = (b == 0 && s > 0) ? 2 : 1;
            const std::string p = "layer" + std::to_string(s + 1) + "." + std::to_string(b) + ".";
            const bool ds = (b == 0) && (stride != 1 || cin != pl * exp);
            const int hout = hcur / stride;
            if (!h->bottleneck) {
                const int T1 = pick({X});
                c = pb.conv(p + "conv1", p + "bn1", cin, w, 3, stride, 1, hcur, 1);
                pb.conv_op(c, X, T1);
                int res = X, T2 = -100;
                if (ds) {
                    T2 = pick({X, T1});
                    c = pb.conv(p + "downsample.0", p + "downsample.1", cin, w * exp, 1, stride, 0, hcur, 0);
                    pb.conv_op(c, X, T2);
                    res = T2;
                }
                const int O = pick({X, T1, T2});
                c = pb.conv(p + "conv2", p + "bn2", w, w, 3, 1, 1, hout, 1, 1);
                pb.conv_op(c, T1, O, res);
                X = O;
            } else {
                BlockRec R{-1, -1, -1, -1, hcur};
                const int T1 = pick({X});
                R.c1 = c = pb.conv(p + "conv1", p + "bn1", cin, w, 1, 1, 0, hcur, 1);
                pb.conv_op(c, X, T1);
                const int T2 = pick({X, T1});
                R.c2 = c = groups > 1 ? pb.gconv(p + "conv2", p + "bn2", w, groups, stride, hcur) : pb.conv(p + "conv2", p + "bn2", w, w, 3, stride, 1, hcur, 1);
                pb.conv_op(c, T1, T2);
                int res = X, dsc = -1;
                if (ds) {
                    const int T3 = pick({X, T1, T2});
                    R.ds = dsc = pb.conv(p + "downsample.0", p + "downsample.1", cin, pl * exp, 1, stride, 0, hcur, 0);
                    pb.conv_op(dsc, X, T3);
                    res = T3;
                }
                R.c3 = c = pb.conv(p + "conv3", p + "bn3", w, pl * exp, 1, 1, 0, hout, 1, 1);
                pb.conv_op(c, T2, T1, res, ds ? X : BUF_NONE);   // T1 is dead after conv2
                if (ds) pb.link_downsample(c, dsc);
                blocks.push_back(R);
                X = T1;
            }
            cin = pl * exp;
            hcur = hout;
        }
    }
    // Block-tail plan (mpx_btail.h): a block whose conv2 is 64 -> 64 3x3 stride 1 on a 56x56 map, whose conv3 is 64 -> 256 and
    // whose successor starts with a 1x1 stride-1 conv 256 -> 64 / 128 (layer1 of ResNet-50 / 101 / 152) runs conv2, conv3 (+ the
    // identity or the K-concatenated downsample branch) and the successor's conv1 as ONE launch.  Four distinct buffers are live
    // across such a launch (block input, t1, block output, next t1): other workgroups still read t1's halo while this one writes.
    {
        auto tail_ok = [&](size_t k) {
            if (k + 1 >= blocks.size()) return false;
            const mpx_conv_desc& d2 = h->convs[blocks[k].c2].d;
            const mpx_conv_desc& d3 = h->convs[blocks[k].c3].d;
            const mpx_conv_desc& n1 = h->convs[blocks[k + 1].c1].d;
            if (!(d2.cin == BT_MID && d2.cout == BT_MID && d2.ksize == 3 && d2.stride == 1 && d2.hin == 56)) return false;
            if (!(d3.cin == BT_MID && d3.cout == BT_OUT)) return false;
            if (blocks[k].ds >= 0) {
                const mpx_conv_desc& dd = h->convs[blocks[k].ds].d;
                if (!(dd.cin == BT_MID && dd.stride == 1 && dd.ksize == 1)) return false;
            }
            return n1.cin == BT_OUT && n1.ksize == 1 && n1.stride == 1 && n1.hin == 56 && (n1.cout == 64 || n1.cout == 128) &&
                   !(blocks[k].ds >= 0 && n1.cout != 64);
        };
        // Pointwise-tail plan (mpx_btail.h, BtPwCfg): a plain block (no downsample branch) whose conv3 is 128 -> 512 and whose successor
        // starts with a 1x1 stride-1 conv 512 -> 128 (layer2's blocks 1 .. n-2) runs conv3 + identity and the successor's conv1 as ONE
        // launch.  Four distinct buffers again: t2, the identity, the block output, the next t1.
        auto ptail_ok = [&](size_t k) {
            if (k + 1 >= blocks.size() || blocks[k].ds >= 0 || tail_ok(k)) return false;
            const mpx_conv_desc& d3 = h->convs[blocks[k].c3].d;
            const mpx_conv_desc& n1 = h->convs[blocks[k + 1].c1].d;
            return d3.cin == BtPw128::MID && d3.cout == BtPw128::OUT && d3.ksize == 1 && d3.stride == 1 && d3.residual == 1 &&
                   n1.cin == BtPw128::OUT && n1.cout == BtPw128::C1 && n1.ksize == 1 && n1.stride == 1 && n1.hin == d3.hin;
        };
        bool any = false;
        for (size_t k = 0; k < blocks.size(); ++k) any |= tail_ok(k);
        // one launch plan: layer1's block tails as OP_BTAIL (bt), layer2's pointwise tails as OP_PTAIL (pt); rec_bt / rec_pt: this plan is the
        // one that fills h->tails / h->ptails (each list once: the other plans number their launches the same way)
        auto plan = [&](std::vector<Op>& out, bool bt, bool pt, bool rec_bt, bool rec_pt) {
            size_t n_bt = 0, n_pt = 0;
            out.push_back(h->ops[0]);       // stem conv, max pool
            out.push_back(h->ops[1]);
            int Xb = BUF_STEM, T1c = -100;         // T1c: buffer of a t1 that the previous tail launch has already written
            for (size_t k = 0; k < blocks.size(); ++k) {
                const BlockRec& R = blocks[k];
                int T1 = T1c;
                // a tail with a downsample branch (layer1.0) runs its block's own conv1 too, on the patch of the block input: no conv1
                // launch, no t1 tensor (in = BUF_NONE)
#ifdef BT_NO_HEAD       // probe builds (tools/ab_lib.sh): layer1.0.conv1 stays a launch of its own
                const bool whole = false;
#else
                const bool whole = bt && tail_ok(k) && R.ds >= 0 && T1 < 0;
#endif
                if (T1 < 0 && !whole) {
                    T1 = pick({Xb});
                    out.push_back(Op{OP_CONV, R.c1, Xb, T1, BUF_NONE, 0, 0, BUF_NONE});
                }
                T1c = -100;
                if (bt && tail_ok(k)) {
                    if (rec_bt) {
                        TailBlock tb;
                        tb.c1 = R.c1; tb.c2 = R.c2; tb.c3 = R.c3; tb.ds = R.ds; tb.next1 = blocks[k + 1].c1;
                        h->tails.push_back(tb);
                    }
                    if (whole) T1 = BUF_NONE;
                    const int O = pick({Xb, T1}), Z = pick({Xb, T1, O});
                    Op o{OP_BTAIL, (int)n_bt++, T1, O, Xb, 0, 0, BUF_NONE};
                    o.z = Z;
                    out.push_back(o);
                    Xb = O;
                    T1c = Z;
                    continue;
                }
                const int T2 = pick({Xb, T1});
                out.push_back(Op{OP_CONV, R.c2, T1, T2, BUF_NONE, 0, 0, BUF_NONE});
                if (pt && ptail_ok(k)) {
                    if (rec_pt) h->ptails.push_back(PointTail{R.c3, blocks[k + 1].c1});
                    const int O = pick({Xb, T2}), Z = pick({Xb, T2, O});
                    Op o{OP_PTAIL, (int)n_pt++, T2, O, Xb, 0, 0, BUF_NONE};
                    o.z = Z;
                    out.push_back(o);
                    Xb = O;
                    T1c = Z;
                    continue;
                }
                int res = Xb;
                if (R.ds >= 0) {
                    const int T3 = pick({Xb, T1, T2});
                    out.push_back(Op{OP_CONV, R.ds, Xb, T3, BUF_NONE, 0, 0, BUF_NONE});
                    res = T3;
                }
                out.push_back(Op{OP_CONV, R.c3, T2, T1, res, 0, 0, R.ds >= 0 ? Xb : BUF_NONE});
                Xb = T1;
            }
            return Xb;
        };
        bool any_pt = false;
        for (size_t k = 0; k < blocks.size(); ++k) any_pt |= ptail_ok(k);
        if (any) h->ops_bt_x = plan(h->ops_bt, true, false, true, false);
        if (any_pt) {       // (an arch with pointwise tails and no block tails gets ops_pt0 alone: mpx_forward never picks ops_pt then)
            h->ops_pt0_x = plan(h->ops_pt0, false, true, false, true);
            if (any) h->ops_pt_x = plan(h->ops_pt, true, true, false, false);
        }
    }
    h->feat = cin;
    pb.op(OP_AVGPOOL, -1, X, BUF_POOL, BUF_NONE, hcur, cin);
    pb.conv_op(pb.conv(conv_spec("fc", "", cin, MPX_NUM_CLASSES, 1, 1, 0, 1, 0).logits()), BUF_POOL, BUF_NONE);
    pb.head();
    for (auto lx : {std::make_pair(&h->ops_bt, h->ops_bt_x), std::make_pair(&h->ops_pt, h->ops_pt_x), std::make_pair(&h->ops_pt0, h->ops_pt0_x)}) {
        if (lx.first->empty()) continue;
        lx.first->push_back(Op{OP_AVGPOOL, -1, lx.second, BUF_POOL, BUF_NONE, hcur, cin, BUF_NONE});
        lx.first->push_back(h->ops[h->ops.size() - 2]);
        lx.first->push_back(h->ops[h->ops.size() - 1]);
    }
    return 0;
}

// The plan as text (mpx_describe_plan): one record per line, "<section> [<index>] key=value ...", every field a build_topology* assigns
// and nothing an engine fills later (no pointer, no device property).  The section is a line's first word.
struct PlanText {
    std::string s;
    void begin(const char* section, int index = -1) {
        s += section;
        if (index >= 0) s += " " + std::to_string(index);
    }
    void kv(const char* key, long long v) { s += std::string(" ") + key + "=" + std::to_string(v); }
    void ks(const char* key, const char* v) { s += std::string(" ") + key + "=" + v; }
    void end() { s += "\n"; }
};

std::string describe_plan(const mpx_engine& e) {
    PlanText t;
    t.begin("engine");
    t.kv("img", e.img); t.kv("in_ch", e.in_ch); t.kv("ncls", e.ncls); t.kv("logit_pitch", e.logit_pitch);
    t.kv("small", e.small); t.kv("densenet", e.densenet); t.kv("googlenet", e.googlenet); t.kv("regnet_y", e.regnet_y);
    t.kv("vit", e.vit); t.kv("vit_T", e.vit_T); t.kv("vit_D", e.vit_D);
    t.kv("n_act_bufs", e.n_act_bufs); t.kv("act_elems_per_image", (long long)e.act_elems_per_image);
    for (int b = 0; b < 4; ++b) t.kv(("act_elems_buf" + std::to_string(b)).c_str(), (long long)e.act_elems_buf[b]);
    t.kv("bottleneck", e.bottleneck); t.kv("feat", e.feat); t.kv("se_pitch_max", e.se_pitch_max);
    t.kv("ops_bt_x", e.ops_bt_x); t.kv("ops_pt_x", e.ops_pt_x); t.kv("ops_pt0_x", e.ops_pt0_x);
    t.end();
    for (size_t i = 0; i < e.convs.size(); ++i) {
        const ConvLayer& L = e.convs[i];
        t.begin("conv", (int)i);
        t.ks("name", L.d.name); t.ks("bn_name", L.d.bn_name);
        t.kv("cin", L.d.cin); t.kv("cout", L.d.cout); t.kv("ksize", L.d.ksize); t.kv("stride", L.d.stride); t.kv("pad", L.d.pad);
        t.kv("hin", L.d.hin); t.kv("hout", L.d.hout); t.kv("relu", L.d.relu); t.kv("residual", L.d.residual);
        t.kv("k_packed", L.d.k_packed); t.kv("cout_pad", L.d.cout_pad);
        t.kv("is_fc", L.is_fc); t.kv("is_stem", L.is_stem); t.kv("consumer_act", L.consumer_act); t.kv("rows", L.rows);
        t.kv("epi_act", L.epi_act); t.kv("has_bias", L.has_bias); t.kv("cin_pad", L.cin_pad); t.kv("cout_store", L.cout_store);
        t.kv("y_pitch", L.y_pitch); t.kv("y_offset", L.y_offset); t.kv("x_pitch", L.x_pitch); t.kv("x_offset", L.x_offset);
        t.kv("in_bf", L.in_bf); t.kv("in_hp", L.in_hp); t.kv("groups", L.groups); t.kv("gw", L.gw);
        t.kv("tile", L.tile); t.kv("tile_default", L.tile_default); t.kv("fuse_partner", L.fuse_partner); t.kv("fuse_main", L.fuse_main);
        t.end();
    }
    const std::pair<const char*, const std::vector<Op>*> lists[] = {{"ops", &e.ops}, {"ops_bt", &e.ops_bt}, {"ops_pt", &e.ops_pt}, {"ops_pt0", &e.ops_pt0}};
    for (const auto& l : lists)
        for (size_t i = 0; i < l.second->size(); ++i) {
            const Op& o = (*l.second)[i];
            t.begin(l.first, (int)i);
            t.kv("kind", o.kind); t.kv("conv", o.conv); t.kv("in", o.in); t.kv("out", o.out); t.kv("res", o.res);
            t.kv("hin", o.hin); t.kv("c", o.c); t.kv("in2", o.in2); t.kv("z", o.z); t.kv("g", o.g); t.kv("ctot", o.ctot);
            t.end();
        }
    for (size_t i = 0; i < e.tails.size(); ++i) {
        const TailBlock& b = e.tails[i];
        t.begin("tail", (int)i);
        t.kv("c1", b.c1); t.kv("c2", b.c2); t.kv("c3", b.c3); t.kv("ds", b.ds); t.kv("next1", b.next1);
        t.end();
    }
    for (size_t i = 0; i < e.ptails.size(); ++i) {
        t.begin("ptail", (int)i);
        t.kv("c3", e.ptails[i].c3); t.kv("next1", e.ptails[i].next1);
        t.end();
    }
    for (size_t i = 0; i < e.norms.size(); ++i) {
        const mpx_norm_desc& d = e.norms[i].d;
        t.begin("norm", (int)i);
        t.ks("name", d.name); t.kv("channels", d.channels); t.kv("hw", d.hw);
        t.end();
    }
    for (size_t i = 0; i < e.dws.size(); ++i) {
        const DwLayer& D = e.dws[i];
        t.begin("dw", (int)i);
        t.ks("name", D.d.name); t.ks("bn_name", D.d.bn_name);
        t.kv("channels", D.d.channels); t.kv("pitch", D.d.pitch); t.kv("stride", D.d.stride); t.kv("hin", D.d.hin); t.kv("clamp_in", D.d.clamp_in);
        t.kv("linear", D.linear); t.kv("in_bf", D.in_bf); t.kv("in_hp", D.in_hp); t.kv("ksize", D.ksize); t.kv("mb", D.mb);
        t.kv("act_in", D.act_in); t.kv("act_out", D.act_out); t.kv("ln", D.ln);
        t.end();
    }
    for (size_t i = 0; i < e.lnorms.size(); ++i) {
        const mpx_lnorm_desc& d = e.lnorms[i].d;
        t.begin("lnorm", (int)i);
        t.ks("name", d.name); t.kv("channels", d.channels); t.kv("hw", d.hw);
        t.end();
    }
    for (size_t i = 0; i < e.attns.size(); ++i) {
        const mpx_attn_desc& d = e.attns[i].d;
        t.begin("attn", (int)i);
        t.ks("name", d.name); t.kv("tokens", d.tokens); t.kv("heads", d.heads); t.kv("head_dim", d.head_dim);
        t.end();
    }
    for (size_t i = 0; i < e.ses.size(); ++i) {
        const SeLayer& E = e.ses[i];
        t.begin("se", (int)i);
        t.ks("name", E.d.name); t.kv("channels", E.d.channels); t.kv("pitch", E.d.pitch); t.kv("q", E.d.q); t.kv("hw", E.d.hw); t.kv("relu", E.relu);
        t.end();
    }
    for (size_t i = 0; i < e.shuffles.size(); ++i) {
        const ShuffleOp& o = e.shuffles[i];
        t.begin("shuffle", (int)i);
        t.kv("side", o.side); t.kv("bf", o.bf); t.kv("hp", o.hp); t.kv("a_pitch", o.a_pitch); t.kv("b_pitch", o.b_pitch); t.kv("b_offset", o.b_offset);
        t.end();
    }
    for (size_t i = 0; i < e.pools3c.size(); ++i) {
        const ClipPool& o = e.pools3c[i];
        t.begin("pool3c", (int)i);
        t.kv("hin", o.hin); t.kv("stride", o.stride); t.kv("pad", o.pad); t.kv("pitch", o.pitch);
        t.end();
    }
    return t.s;
}

// mpx_describe_plan's body: a throw-away engine on the host, the build_topology that mpx_create runs, the text.
int describe_plan_of(int arch_id, char* buf, size_t cap, size_t* len) {
    if (!len) return MPX_E_ARG;
    *len = 0;
    mpx_engine e;
    e.arch = arch_id; e.max_batch = 1;
    const int rc = build_topology(&e);
    if (rc) return rc;
    const std::string s = describe_plan(e);
    *len = s.size();
    if (!buf) return 0;
    if (cap <= s.size()) return MPX_E_ARG;
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
}

}  // namespace
