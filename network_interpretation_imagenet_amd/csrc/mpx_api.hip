// mpx_api.hip -- C-ABI (include/mpx.h) + host-side engine: topology, weight packing, workspace,
// launch sequencing.  Compiled for gfx950 only:  hipcc --offload-arch=gfx950 -shared -fPIC.
#include "../../include/mpx.h"
#include "mpx_kernels.h"
#include "mpx_conv3p.h"
#include "mpx_conv3pp.h"
#include "mpx_conv256.h"
#include "mpx_conv256p.h"
#include "mpx_convx.h"
#include "mpx_convw.h"
#include "mpx_btail.h"
#include "mpx_stemtab.h"
#include "mpx_dw.h"
#include "mpx_fire.h"
#include "mpx_pool3c.h"
#include "mpx_shuffle.h"
#include "mpx_mbconv.h"
#include "mpx_gconv.h"
#include "mpx_gconvw.h"
#include "mpx_cnext.h"
#include "mpx_attn.h"
#include "mpx_softmask.h"
#include "mpx_saliency_classes.h"
#include "mpx_occlusion.h"
#include "mpx_cam.h"
#include "mpx_rankmask.h"
#include "mpx_surrogate.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <initializer_list>
#include <new>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mpx;

namespace {

constexpr int kActBufs = 4;
constexpr int kStemK = 7;
constexpr int kProfilePairs = 4096;
constexpr size_t kActElemsPerImage = 112 * 112 * 64;   // ImageNet: largest activation (stem output, = 56*56*256)
constexpr size_t kVggActElemsPerImage = 224 * 224 * 64; // VGG: the 64-channel maps of the first stage
constexpr size_t kAlexActElemsPerImage = 55 * 55 * 64;  // AlexNet: the output of features.0
constexpr size_t kMobileActElemsPerImage = 112 * 112 * 96;   // MobileNetV2: features.2's expanded map, 1.5 x kActElemsPerImage
constexpr size_t kSqueezeActElemsPerImage = 111 * 111 * 64;  // SqueezeNet 1.1: the output of features.0 (the largest concatenation is 55 * 55 * 128)
constexpr size_t kShuffleActElemsPerImage = 112 * 112 * 32; // ShuffleNetV2: conv1's output, 24 channels at pitch 32 (= x2_0's stage2.0.branch2.0 map, 56 * 56 * 128)
constexpr size_t kEffActElemsPerImage = 112 * 112 * 96;  // EfficientNet-B0: features.2.0's expanded map (= MobileNetV2's buffer)
constexpr size_t kCnextActElemsPerImage = 56 * 56 * 384;  // ConvNeXt: block.3's output in stage 0 (the same number of elements again)
constexpr int kVitWidth = 768, kVitHeads = 12, kVitMlp = 3072, kVitLayers = 12;     // torchvision vit_b_16 / vit_b_32
constexpr int kSmallCPad = 32;                         // small nets: channels are stored padded to a multiple of 32

enum OpKind { OP_CONV = 0, OP_MAXPOOL = 1, OP_AVGPOOL = 2, OP_HEAD = 3, OP_AVGPAD = 4, OP_BTAIL = 5, OP_MAXPOOL2 = 6, OP_MAXPOOL3P0 = 7,
              OP_CATNORM = 8, OP_AVGPOOL2 = 9, OP_DWCONV = 10, OP_AVGPOOL6 = 11, OP_AVGLOGITS = 12, OP_MAXPOOL3C = 13, OP_SHUFFLE = 14,
              OP_SEGATE = 15, OP_SESCALE = 16, OP_AVGPOOLSILU = 17, OP_PTAIL = 18, OP_LNORM = 19, OP_AVGPOOLLN = 20,
              OP_TOKENS = 21, OP_ATTN = 22, OP_LNORMROWS = 23 };
enum Buf { BUF_INPUT = -1, BUF_POOL = -2, BUF_NONE = -3, BUF_STEM = -4 };   // BUF_STEM: the pooled stem output (planes of its own)

struct ConvLayer {
    mpx_conv_desc d;
    half_t* w_hi = nullptr;
    half_t* w_lo = nullptr;
    float* scale = nullptr;
    float* shift = nullptr;
    bool loaded = false;
    bool is_fc = false;
    bool is_stem = false;
    int consumer_act = 0;   // 1: torchvision follows this conv with SiLU, which its one consumer takes on load (mpx_dw.h); relu is 0 then
    int rows = 0;           // > 0: a token layer (ViT): the layer runs on `rows` = T rows per image that are no square map -- d.hin = d.hout = 0
                            // and conv_params hands the kernels hin = ho = rows, win = wo = 1 (mpx_conv_rows)
    int epi_act = 0;        // 1: exact GELU in the epilogue (a ConvNeXt block.3: ConvGelu, mpx_conv.h); the layer runs the generic tiles only
    bool has_bias = false;  // the reference module is nn.Conv2d(bias=True) (small nets): state_dict has <name>.bias
    int cin_pad = 0;        // channels per pixel of the input planes (= cin except for the small nets, which pad to 32)
    int cout_store = 0;     // channels per pixel of the output planes (row pitch and store bound)
    // output slice (a SqueezeNet expand conv: half of its Fire module's concatenation; a GoogLeNet branch's last conv: one of the four ranges of
    // its Inception module's): the layer writes channels [y_offset, y_offset + cout_store) of planes whose pixels are y_pitch channels apart, on
    // the SLICE form of the generic kernel (mpx_conv.h).  Any (y_pitch, y_offset, cout_store) that are multiples of 8 with y_offset + cout_store
    // <= y_pitch; cout_store may exceed cout (rows of zero weights, scale and shift: exact zeros), which is how inception4d's 528-channel
    // concatenation gets its 16 pad channels written.  y_pitch = 0: an ordinary layer, which fills whole pixel rows of cout_store channels.
    int y_pitch = 0;
    int y_offset = 0;
    // input slice (a stride-1 ShuffleNetV2 block's branch2.0: the second half of a two-half stage map, read in place): the layer reads channels
    // [x_offset, x_offset + cin_pad) of planes whose pixels are x_pitch channels apart -- the generic kernel's pix_stride, which it carries
    // separately from k_per_tap.  x_pitch = 0: an ordinary layer, which reads whole pixel rows of cin_pad channels.
    int x_pitch = 0;
    int x_offset = 0;
    // input in the two-half layout (mpx_shuffle.h): the layer reads a whole stage map of 2 * in_bf logical channels stored with pitch
    // 2 * in_hp = cin_pad; the packer puts logical weight column l at l (l < in_bf) or in_hp + l - in_bf.  in_hp = 0: columns as they come.
    int in_bf = 0;
    int in_hp = 0;
    int groups = 1;         // > 1: a grouped 3x3 layer (a ResNeXt conv2: cin = cout = the width, cin / groups channels per group), whose packed planes
                            // are mpx_gconv.h's -- cout_pad = cout rows of k_packed = gconv_kp(max(cin / groups, 16)), the K of ONE channel block
    bool gw = false;        // a grouped layer in mpx_gconvw.h's form (a RegNetX / RegNetY f.b: any group count, cin / groups = 16, 24, 48, 56 or 120, planes at a
                            // pitch of cin_pad / cout_store >= the width): packed planes [groups][ceil(cg / 16)][k_packed / 32][64][8], i.e.
                            // cout_pad = groups * ceil(cg / 16) * 16 rows of k_packed = gconvw_kp(cg).  Runs tile 18, and tile 16 where that accepts it
    int tile = 0;           // ConvTile<n> variant (mpx_set_conv_tile)
    int tile_default = -1;  // the layer's default where the topology sets one of its own (DenseNet's conv2); -1: default_tile(d)
    // downsample fusion (bottleneck blocks): the block's last 1x1 conv ("main") and its downsample 1x1 conv ("ds")
    // run as ONE launch over the K-concatenation [W3 * s3/s | Wds * sds/s] (build_fused)
    int fuse_partner = -1;  // main -> ds layer index, ds -> main layer index
    bool fuse_main = false;
    half_t* fw_hi = nullptr;    // main only: fused planes [cout_pad][k1 + k2]
    half_t* fw_lo = nullptr;
    float* fscale = nullptr;
    float* fshift = nullptr;
    bool fused_loaded = false;
    std::vector<float> hw, hgamma, hbeta, hmean, hvar;   // host copies of a fusable layer's tensors (until both are in)
    float heps = 0.f;
};

struct Op {
    int kind;
    int conv;       // layer index for OP_CONV
    int in, out, res;
    int hin, c;     // pools
    int in2;        // fused main conv: buffer of the block input (the downsample branch's operand), else BUF_NONE
    int z = BUF_NONE;   // OP_BTAIL: buffer of the next block's conv1 output; `conv` = index into mpx_engine::tails,
                        // in = t1, res = block input / identity, out = block output
                        // OP_PTAIL: the same with `conv` = index into mpx_engine::ptails and in = t2
    int g = 0, ctot = 0;    // OP_CATNORM (DenseNet): `conv` = index into mpx_engine::norms, in = the fresh g channels, res = the block's raw
                            // concatenation (ctot channels per pixel), out = the normalised first c channels, hin = the map's side
};

// A BatchNorm that precedes its conv (DenseNet: every norm1, each transition's norm, norm5): fp32 scale / shift vectors of its own.
struct NormLayer {
    mpx_norm_desc d;
    float* scale = nullptr;
    float* shift = nullptr;
    bool loaded = false;
};

// A 64-channel bottleneck block whose tail runs as ONE launch (mpx_btail.h): conv2 -> conv3 (+ identity or K-concatenated
// downsample branch) -> the next block's conv1.  Weights: conv2's and next1's packed planes as they are; conv3's (or the fused
// conv3 | downsample planes') with columns [0,64) K-permuted into planes of its own.
struct TailBlock {
    int c1 = -1, c2 = -1, c3 = -1, ds = -1, next1 = -1;     // c1: the block's own conv1 (runs inside the launch when the block has a downsample branch)
    half_t* w3p_hi = nullptr;
    half_t* w3p_lo = nullptr;
    bool ready = false;
};

// A plain 128 -> 512 bottleneck block whose conv3 + identity runs with the next block's conv1 (512 -> 128) as ONE launch (mpx_btail.h,
// the pointwise form).  It reads the packed planes of its two layers as they are: no copy to keep in step with a reload.
struct PointTail {
    int c3 = -1, next1 = -1;
};

// A depthwise 3x3 conv + BatchNorm + ReLU6 (MobileNetV2; mpx_dw.h): fp32 tap-major weights [9][pitch] and BatchNorm vectors of its own.
struct DwLayer {
    mpx_dwconv_desc d;
    bool linear = false;    // ShuffleNetV2: BatchNorm only, no activation and no clamp (the run form without SiLU, mpx_dw.h)
    int in_bf = 0, in_hp = 0;   // its planes are a two-half stage map (channels = 2 * in_bf, pitch = 2 * in_hp): logical channel c loads to its physical position
    int ksize = 3;          // 3 or 5 (EfficientNet-B0): weights [ksize * ksize][pitch]
    bool mb = false;        // EfficientNet-B0: the run form (mpx_dw.h) with SiLU on load (act_in) and in the epilogue (act_out)
    int act_in = 0, act_out = 0;
    bool ln = false;        // ConvNeXt: depthwise 7x7 + bias + LayerNorm over the channels (dwconv7x7_ln_kernel, mpx_cnext.h); scale / shift hold the
                            // LayerNorm's weight / bias, `bias` the conv's own bias, `eps` the LayerNorm's epsilon as loaded
    float* bias = nullptr;
    float eps = 0.f;
    float* w = nullptr;
    float* scale = nullptr;
    float* shift = nullptr;
    bool loaded = false;
};

// A LayerNorm over the channels that is a launch of its own (ConvNeXt; mpx_cnext.h): the module's weight and bias as they are
struct LnLayer {
    mpx_lnorm_desc d;
    float* gamma = nullptr;
    float* beta = nullptr;
    float eps = 0.f;
    bool loaded = false;
};

// An attention launch of the op list (ViT; mpx_attn.h): in = the in_proj planes [B][T][3 D], out = planes [B][T][D]
struct AttnLayer {
    mpx_attn_desc d;
};

// A Squeeze-and-Excitation layer (EfficientNet-B0, RegNetY; mpx_mbconv.h): fp32 fc weights and biases of its own, laid out for se_gate_kernel
struct SeLayer {
    mpx_se_desc d;
    float* w1 = nullptr;    // [q][pitch]
    float* b1 = nullptr;    // [q]
    float* w2 = nullptr;    // [q][pitch], j-major
    float* b2 = nullptr;    // [pitch], -inf on the pad channels
    bool relu = false;      // fc1's activation: ReLU (a RegNetY block's f.se) instead of SiLU (mpx_se_act)
    bool loaded = false;
};

// A channel shuffle of the op list (ShuffleNetV2; mpx_shuffle.h): a = Op::in at a_pitch, b = Op::res advanced by b_offset at b_pitch
struct ShuffleOp {
    int side, bf, hp, a_pitch, b_pitch, b_offset;
};

// A clipped-window 3x3 max pool of the op list (GoogLeNet; mpx_pool3c.h)
struct ClipPool {
    int hin, stride, pad, pitch;
};

// The per-family list of the profile that a launch of kind 2 is booked on next to 'pool' (mpx_profile_collect*), in the order of the public
// argument lists; `index` is the launch's position in that list (the engine's norm, depthwise layer, clipped pool ... k; 0 where the family is
// one number).  PF_NONE: no list -- every launch of another kind, every plain pool, and every launch a stand-alone entry makes.
enum ProfFamily { PF_NONE = 0, PF_NORM, PF_AVGPOOL2, PF_DW, PF_POOL3C, PF_SHUFFLE, PF_SE_GATE, PF_SE_SCALE, PF_LNORM, PF_ATTN, PF_TOKENS, PF_COUNT };

struct ProfTag {
    ProfFamily family = PF_NONE;
    int index = 0;
};

struct ProfRec {
    hipEvent_t t0, t1;
    int kind;
    int conv;
    ProfTag tag;
};

}  // namespace

struct mpx_engine {
    int arch = 0, max_batch = 0, device = 0;
    int num_cus = 256;
    // geometry of the network family: ImageNet ResNets (224x224x3, padded NHWC4 staging for the 7x7 stem, 1000 classes) or
    // the reference's two small networks (28x28x1 / 32x32x3, staging [B][H][W][32] read by a generic 3x3 conv, 10 classes)
    int img = MPX_IMG, in_ch = 3, ncls = MPX_NUM_CLASSES, logit_pitch = MPX_NUM_CLASSES;
    bool small = false;
    bool densenet = false;          // torchvision DenseNet (growth rate 32): the ResNet stem shape, dense blocks over a raw concatenation
    std::vector<NormLayer> norms;   // its stand-alone BatchNorms in forward order
    std::vector<DwLayer> dws;       // the depthwise layers in forward order (MobileNetV2, ShuffleNetV2, EfficientNet-B0, ConvNeXt)
    bool googlenet = false;         // torchvision GoogLeNet: Inception modules over three activation buffers, staged through K0 only
    std::vector<ClipPool> pools3c;  // its clipped-window 3x3 max pools in forward order
    std::vector<ShuffleOp> shuffles;    // ShuffleNetV2's channel shuffles in forward order
    std::vector<SeLayer> ses;       // the Squeeze-and-Excitation layers in forward order (EfficientNet-B0, RegNetY)
    float* se_gate = nullptr;       // f32[max_batch][se_pitch_max]: the gates of the SE layer in flight
    int se_pitch_max = 0;
    std::vector<LnLayer> lnorms;    // the stand-alone LayerNorms in forward order (ConvNeXt, ViT)
    bool regnet_y = false;          // torchvision RegNetY 800MF .. 8GF (a RegNetX trunk, build_topology_regnet): an SE gate with ReLU between f.b and f.c of every block
    bool vit = false;               // torchvision vit_b_16 / vit_b_32: an encoder over four activation buffers of sizes of their own, staged through K0 only
    int vit_T = 0, vit_D = 0;       // tokens per image (197 / 50) and width (768)
    std::vector<AttnLayer> attns;   // its attention launches in forward order
    float* cls_token = nullptr;     // DEV f32[D]: class_token
    float* pos_emb = nullptr;       // DEV f32[T][D]: encoder.pos_embedding
    bool tokens_loaded = false;
    size_t act_elems_buf[4] = {0, 0, 0, 0};     // elements per image of each activation buffer where they differ (ViT); 0: act_elems_per_image
    int n_act_bufs = kActBufs;      // activation buffers the op list uses (mpx_create allocates these only)
    size_t act_elems_per_image = 0;
    float* k0_scratch = nullptr;    // small nets: f32[2 + 4096 + max_batch]: image min, max-min, per-superpixel max, per-mask max
    bool bottleneck = false;
    int feat = 0;
    std::vector<ConvLayer> convs;
    std::vector<Op> ops;
    std::vector<Op> ops_bt;         // the same network with layer1's block tails as OP_BTAIL (empty if the arch has none)
    std::vector<TailBlock> tails;
    int ops_bt_x = 0;               // buffer of the last block's output in ops_bt
    bool fuse_bt = true;            // mpx_forward uses ops_bt when every tail is ready (mpx_set_fusion bit 1)
    std::vector<Op> ops_pt;         // ops_bt with layer2's pointwise tails as OP_PTAIL (empty if the arch has none)
    std::vector<Op> ops_pt0;        // ops with them (the block tails are off or overridden by a tile)
    std::vector<PointTail> ptails;
    int ops_pt_x = 0, ops_pt0_x = 0;
    bool fuse_pt = true;            // mpx_forward uses ops_pt / ops_pt0 (mpx_set_fusion bit 2; needs bit 0)
    const std::vector<Op>* fwd_ops = nullptr;   // the op list the last mpx_forward ran (mpx_pool_input: where that forward's pool read)
    char* arena = nullptr;
    size_t arena_bytes = 0;
    char* tab_arena = nullptr;      // the stem table of one image (CSR, heavy-pixel list, bit planes): allocated by the FIRST mpx_stem_table_build
    size_t tab_arena_bytes = 0;
    half_t* in_hi = nullptr;
    half_t* in_lo = nullptr;
    half_t* act_hi[kActBufs] = {};
    half_t* act_lo[kActBufs] = {};
    half_t* pool_hi = nullptr;
    half_t* pool_lo = nullptr;
    float* logits = nullptr;
    float* seg_scratch = nullptr;   // f32[4096] per-superpixel counts (K5)
    // the stem by superposition (mpx_stemtab.h; ImageNet ResNets): pooled stem output planes [max_batch][56][56][64] of their own (written by
    // the stem + pool launch or by mpx_stem_table_apply), ONE image's table, the bit planes of a staging call's mask rows
    half_t* stem_hi = nullptr;
    half_t* stem_lo = nullptr;
    float* stem_w32 = nullptr;      // [147][64] fp32 stem weights, tap-major
    float* stem_s32 = nullptr;      // [64] gamma / sqrt(var + eps)
    float* stem_t32 = nullptr;      // [64] beta - mean * scale
    int* tab_cnt = nullptr;
    int* tab_off = nullptr;
    int* tab_lab = nullptr;
    int* tab_heavy = nullptr;       // [56 * 56 + 1]: the heavy pooled pixels of the table in place, last element = their number
    float* tab_vec = nullptr;
    unsigned* tab_bits = nullptr;   // [4096][ceil(max_batch / 32) + 1]
    size_t tab_sizes[4] = {0, 0, 0, 0};   // bytes of one int vector / lab / vec / bits (mpx_create), taken from tab_arena on first use
    int tab_S = -1;                 // S of the table in place (-1: none)
    bool stem_w_loaded = false;
    std::vector<uint8_t> slot_src;  // per input slot: 0 = never staged, 1 = K0 (input staging), 2 = stem table (pooled planes)
    std::string err;
    bool in_forward = false;
    unsigned last_kernels = 0;      // bit t: the last conv call launched the kernel of tile id t (mpx_last_conv_kernels)
    bool fuse_ds = true;    // mpx_forward runs a block's last conv and its downsample conv as one launch (mpx_set_fusion)
    bool fuse_pool = true;  // ... and the ImageNet stem conv with its 3x3 stride-2 max pool (mpx_stem_conv_maxpool)
    bool prof_on = false;
    std::vector<ProfRec> prof_pool;
    int prof_used = 0;
    hipStream_t prof_stream = nullptr;
#ifdef MPX_DIAG
    unsigned long long* stamps = nullptr;
#endif
};

namespace {

int fail(mpx_engine* h, int code, const char* fmt, ...) {
    if (h) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        h->err = buf;
    }
    return code;
}

#define MPX_HIP(h, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((h), (int)e_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),     \
                        __FILE__, __LINE__);                                                     \
    } while (0)

// every entry point selects the engine's device; mpx_forward does it ONCE and runs its ~110 launches without the call
#define MPX_SET_DEVICE(h)                                   \
    do {                                                    \
        if (!(h)->in_forward) MPX_HIP((h), hipSetDevice((h)->device)); \
    } while (0)

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

void set_name(char* dst, const std::string& s) {
    std::snprintf(dst, 48, "%s", s.c_str());
}

constexpr int kGconvTile = 16;      // the grouped 3x3 kernel (mpx_gconv.h); ids 15 and 17 stay unassigned
constexpr int kGconvwTile = 18;     // the grouped 3x3 kernel for any group count, width and pitch (mpx_gconvw.h)

uint16_t half_bits(half_t v) {
    uint16_t u;
    std::memcpy(&u, &v, 2);
    return u;
}

hipStream_t as_stream(void* s) { return (hipStream_t)s; }

struct ProfScope {
    mpx_engine* h;
    hipStream_t st;
    ProfRec* rec = nullptr;
    ProfScope(mpx_engine* h_, hipStream_t st_, int kind, int conv, ProfTag tag = ProfTag()) : h(h_), st(st_) {
        if (h->prof_on && h->prof_used < (int)h->prof_pool.size()) {
            rec = &h->prof_pool[h->prof_used++];
            rec->kind = kind;
            rec->conv = conv;
            rec->tag = tag;
            h->prof_stream = st;
            (void)hipEventRecord(rec->t0, st);
        }
    }
    ~ProfScope() {
        if (rec) (void)hipEventRecord(rec->t1, st);
    }
};

// ---- conv dispatch ----------------------------------------------------------------------------------------------------------------
// A layer's conv kernel is a tile id (mpx_set_conv_tile).  kTiles below holds one row per product id; a launcher is handed the id whose
// bit of mpx_last_conv_kernels it sets when its own kernel runs, and falls back to other rows by id.

typedef int (*LaunchFn)(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st);
int launch_tile(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st);

// a kernel of tile `id` was launched: the launch error, else bit `id` of mpx_last_conv_kernels
int launched(mpx_engine* h, int id) {
    MPX_HIP(h, hipGetLastError());
    h->last_kernels |= 1u << id;
    return 0;
}

// p.n_tiles_c and the number of TC x TP tiles of a launch (`tiles`), which must fit the packed weight rows and a 32-bit grid
int conv_tiles(mpx_engine* h, ConvParams& p, int cout_pad, int TC, int TP, long long& tiles) {
    p.n_tiles_c = (p.cout + TC - 1) / TC;     // weights are padded to cout_pad >= n_tiles_c * TC rows
    if (p.n_tiles_c * TC > cout_pad) return fail(h, MPX_E_ARG, "conv tile exceeds the packed weight rows");
    tiles = ((long long)p.M + TP - 1) / TP * p.n_tiles_c;
    if (tiles <= 0 || tiles > 0x7fffffffLL) return fail(h, MPX_E_ARG, "conv grid out of range");
    return 0;
}

// Grid of a persistent kernel: one workgroup per CU, a multiple of 8 (XCD classes) and of n_tiles_c (a workgroup keeps its cout tile);
// 0 when the tiles do not fill one such unit.  Each launcher keeps its own threshold under which smaller tiles win.
long long persistent_grid(const mpx_engine* h, const ConvParams& p, long long tiles) {
    const int c = p.n_tiles_c, unit = 8 > c ? (8 % c == 0 ? 8 : 8 * c) : (c % 8 == 0 ? c : 8 * c);
    return std::min<long long>(h->num_cus, tiles) / unit * unit;
}

// Eligibility predicates judge a layer's descriptor (default_tile sees nothing else; eligible() below adds what only the layer knows).
// 256x256 tile (mpx_conv256.h, tile id 9): 1x1 stride-1 layers whose cout is a multiple of 256 and whose K is a multiple of 64
bool conv256_eligible(const mpx_conv_desc& d) {
    return d.ksize == 1 && d.stride == 1 && d.pad == 0 && d.cout % 256 == 0 && d.cin % 64 == 0;
}

// persistent expanding-1x1 kernel (mpx_convx.h, tile id 10): as tile 9 plus K >= 128
bool convx_eligible(const mpx_conv_desc& d) { return conv256_eligible(d) && d.cin >= 128; }

// weights-in-registers expanding-1x1 kernel (mpx_convw.h, tile id 14): tile 10's layers with K = 256 exactly (a wave keeps the
// 64 x 256 x (hi + lo) weights of its channels in 256 VGPRs)
bool convw_eligible(const mpx_conv_desc& d) { return conv256_eligible(d) && d.cin == ConvW::K; }

// persistent 256x256 kernel (mpx_conv256p.h, tile id 13): tile 9's layers without a residual operand
bool conv256p_eligible(const mpx_conv_desc& d) { return conv256_eligible(d) && !d.residual; }

// Rows of the largest input patch any TP-pixel tile of an HxH map needs (mpx_conv3p.h), rounded up to 16.
int patch_rows_needed(int H, int TP) {
    const int W = H, PW = W + 2, PIMG = (H + 2) * PW, howo = H * W;
    auto pb = [&](long long m) { const long long n = m / howo, rem = m % howo; return n * PIMG + (rem / W) * PW + rem % W; };
    long long worst = 0;
    for (long long m0 = 0; m0 < (long long)TP * howo; m0 += TP) {      // the pattern repeats after lcm(TP, H*W) pixels
        const long long r = pb(m0 + TP - 1) - pb(m0) + 2 * PW + 3;
        worst = r > worst ? r : worst;
    }
    return (int)((worst + 15) / 16 * 16);
}

constexpr int kLdsLimit = 160 * 1024;

// 3x3 stride-1 layers whose patch fits the LDS: the patch kernel (tile id 6)
template <class PC>
bool patch_fits(const mpx_conv_desc& d) {
    if (d.ksize != 3 || d.stride != 1 || d.pad != 1 || d.cin % 64 != 0 || d.hin != d.hout) return false;
    const int rows = patch_rows_needed(d.hin, PC::TP);
    return rows <= PC::MAX_PATCH_ROWS && PC::lds_bytes(rows) <= kLdsLimit;
}

bool patch_eligible(const mpx_conv_desc& d) {
    return d.cout <= 64 ? patch_fits<PatchTile1>(d) : (patch_fits<PatchTile0>(d) || patch_fits<PatchTile2>(d));
}

// persistent patch kernel (mpx_conv3pp.h, tile id 12): the patch kernel's layers with cout >= 128 and no residual whose LDS image leaves 1 KB for the
// cout tile's scale / shift vectors
template <class PC>
bool patchp_fits(const mpx_conv_desc& d) {
    return d.cout >= 128 && !d.residual && patch_fits<PC>(d) && PatchPersistent<PC>::lds_bytes(patch_rows_needed(d.hin, PC::TP)) <= kLdsLimit;
}

bool patchp_eligible(const mpx_conv_desc& d) { return patchp_fits<PatchTile0>(d) || patchp_fits<PatchTile2>(d); }

// The generic kernel (mpx_conv.h) on tile Cfg.  With DUAL, a launch whose params carry a K-concatenated second operand (p.k1 > 0,
// launch_conv_fused) runs the dual-operand instantiation.
template <class Cfg, bool DUAL = false>
int launch_conv_tile(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, Cfg::TC, Cfg::TP, tiles)) return rc;
    if (L.y_pitch) {        // an output slice (launch_conv has set p.y_pitch and advanced p.y_*): the SLICE form, whatever else the row offers
        if (p.r_hi || p.y_f32 || p.k1 || p.y_pitch != L.y_pitch)
            return fail(h, MPX_E_INTERNAL, "slice conv: %s takes no residual operand, no fp32 output and no second K segment", L.d.name);
        hipLaunchKernelGGL((conv_f16x3_kernel<Cfg, false, false, true>), dim3((unsigned)tiles), dim3(Cfg::NT), Cfg::LDS, st, p);
        return launched(h, id);
    }
    if (L.epi_act) {        // GELU in the epilogue (a ConvNeXt block.3): the same tile with ACT = 1, whatever else the row offers
        if (L.epi_act != 1 || p.r_hi || p.y_f32 || p.k1 || p.relu)
            return fail(h, MPX_E_INTERNAL, "GELU conv: %s takes no residual operand, no fp32 output, no second K segment and no ReLU", L.d.name);
        hipLaunchKernelGGL((conv_f16x3_kernel<ConvGelu<Cfg>>), dim3((unsigned)tiles), dim3(Cfg::NT), Cfg::LDS, st, p);
        return launched(h, id);
    }
    if constexpr (DUAL) {
        if (p.k1) {
            if (((p.k1 >> 5) - Cfg::NSX) < 0 || (((p.k1 >> 5) - Cfg::NSX) & 1))
                return fail(h, MPX_E_INTERNAL, "dual conv: k1/32 - ring depth must be even and >= 0");
            hipLaunchKernelGGL((conv_f16x3_kernel<Cfg, true>), dim3((unsigned)tiles), dim3(Cfg::NT), Cfg::LDS, st, p);
            return launched(h, id);
        }
    }
    hipLaunchKernelGGL((conv_f16x3_kernel<Cfg>), dim3((unsigned)tiles), dim3(Cfg::NT), Cfg::LDS, st, p);
    return launched(h, id);
}

int launch_conv256(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, Conv256::TC, Conv256::TP, tiles)) return rc;
    hipLaunchKernelGGL(conv256_f16x3_kernel, dim3((unsigned)tiles), dim3(Conv256::NT), Conv256::LDS, st, p);
    return launched(h, id);
}

// a residual operand runs on the 256x256 kernel itself, under one round of tiles the 128x128 kernel (same bits, as launch_convx)
int launch_conv256p(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    if (p.r_hi) return launch_tile(h, 9, L, p, st);
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, Conv256P::TC, Conv256P::TP, tiles)) return rc;
    const long long grid = persistent_grid(h, p, tiles);
    if (grid <= 0 || tiles < h->num_cus) return launch_tile(h, 2, L, p, st);
    hipLaunchKernelGGL(conv256p_f16x3_kernel<false>, dim3((unsigned)grid), dim3(Conv256P::NT), Conv256P::LDS, st, p);
    return launched(h, id);
}

// The DUAL form of the persistent 256x256 kernel: a fused launch (launch_conv_fused) whose main conv is a 1x1 stride-1 layer with
// cout % 256 == 0 and whose two K segments are whole step pairs.  The launch has no residual operand (the identity is inside K), which is
// what kept these layers off tile 13.
bool conv256p_dual_eligible(const ConvLayer& L, const ConvLayer& D) {
    return !L.is_fc && !L.is_stem && L.cin_pad == L.d.cin && D.cin_pad == D.d.cin && conv256_eligible(L.d) && D.d.ksize == 1 && D.d.pad == 0 &&
           D.d.cin % 64 == 0;
}

// 1: the kernel ran (bit 13); 0: the launch has less than one round of tiles and stays with tile 7's dual kernel (BO rounds, small
// batches: the rule and its reason are launch_convx's); < 0: error
int launch_conv256p_dual(mpx_engine* h, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    if (p.k1 <= 0 || p.k1 % 64 != 0 || (p.ktot - p.k1) <= 0 || (p.ktot - p.k1) % 64 != 0 || p.r_hi)
        return fail(h, MPX_E_INTERNAL, "dual 256x256 conv: k1 = %d and k2 = %d must be multiples of 64, without a residual operand", p.k1, p.ktot - p.k1);
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, Conv256P::TC, Conv256P::TP, tiles)) return rc;
    const long long grid = persistent_grid(h, p, tiles);
    if (grid <= 0 || tiles < h->num_cus) return 0;
    hipLaunchKernelGGL(conv256p_f16x3_kernel<true>, dim3((unsigned)grid), dim3(Conv256P::NT), Conv256P::LDS, st, p);
    if (int rc = launched(h, 13)) return rc;
    return 1;
}

int launch_convx(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, ConvX::TC, ConvX::TP, tiles)) return rc;
    const long long grid = persistent_grid(h, p, tiles);
    // less than one round of tiles (small batches: one image's window table, a BO round): the persistent walk would serialise the
    // tiles that do not fill a grid unit, and half-empty CUs gain more from tiles a quarter of the size -- the 128x128 kernel, which
    // sums in the same order (bit-identical).  tools/layer_profile.py, conv ms per forward: batch 29 8.24 -> 3.92, 118 10.28 -> 6.78,
    // 211 13.50 -> 11.62 with this rule on the three persistent kernels
    if (grid <= 0 || tiles < h->num_cus) return launch_tile(h, 7, L, p, st);
    hipLaunchKernelGGL(convx_f16x3_kernel, dim3((unsigned)grid), dim3(ConvX::NT), ConvX::LDS, st, p);
    return launched(h, id);
}

// under two rounds of tiles the 128x128 kernel, as launch_convx
int launch_convw(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    if (p.ktot != ConvW::K) return fail(h, MPX_E_INTERNAL, "convw: K = %d (the kernel holds K = %d in registers)", p.ktot, ConvW::K);
    // The kernel serves what every layer it is the default for asks of it and what the parity tests cover: the residual add + ReLU of a block's
    // last conv.  A call through mpx_conv_bn_act WITHOUT a residual or (no such layer exists in the networks) without ReLU takes tile 10's
    // kernel, which sums in the same order: only <K, RELU = true> is instantiated (the <false> and null-residual paths had no test).
    if (!p.relu || !p.r_hi) return launch_tile(h, 10, L, p, st);
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, ConvW::TC, ConvW::TP, tiles)) return rc;
    const long long grid = persistent_grid(h, p, tiles);
    if (grid <= 0 || tiles < 2LL * h->num_cus) return launch_tile(h, 7, L, p, st);
    // (the kernel is a template over K; K = 128 -- 128 -> 512 on 28 x 28 maps -- was built and measured in round 5: parity green, bit-equal to tile 10, and a
    // tie with it, 7.26 against 7.19 ms for the four layers: two stages of the epilogue slice per MFMA gap do not hide any more.  Only K = 256 is instantiated.)
    hipLaunchKernelGGL((convw_f16x3_kernel<ConvW::K, true>), dim3((unsigned)grid), dim3(ConvW::NT), ConvW::LDS, st, p);
    return launched(h, id);
}

template <class PC>
int launch_conv_patch(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, PC::TC, PC::TP, tiles)) return rc;
    p.patch_rows = patch_rows_needed(L.d.hin, PC::TP);
    hipLaunchKernelGGL(conv3x3p_f16x3_kernel<PC>, dim3((unsigned)tiles), dim3(PC::NT), PC::lds_bytes(p.patch_rows), st, p);
    return launched(h, id);
}

// under one round of tiles, with a residual operand or past 2^23 padded pixels the patch kernel of the same tile (tile 6, same bits)
template <class PC>
int launch_conv_patchp(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    long long tiles;
    if (int rc = conv_tiles(h, p, L.d.cout_pad, PC::TC, PC::TP, tiles)) return rc;
    const long long grid = persistent_grid(h, p, tiles);
    // (the kernel divides pixel and padded-pixel indices with a float reciprocal: exact below 2^23)
    const int H = L.d.hin;
    const long long padded = (long long)(p.M / (H * H) + 2) * (H + 2) * (H + 2);
    if (grid <= 0 || tiles < h->num_cus || p.r_hi || padded >= (1 << 23)) return launch_conv_patch<PC>(h, 6, L, p, st);
    p.patch_rows = patch_rows_needed(H, PC::TP);
    hipLaunchKernelGGL(conv3x3pp_f16x3_kernel<PC>, dim3((unsigned)grid), dim3(PC::NT), PatchPersistent<PC>::lds_bytes(p.patch_rows), st, p);
    return launched(h, id);
}

int launch_patch(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    if (L.d.cout <= 64) return launch_conv_patch<PatchTile1>(h, id, L, p, st);
    return patch_fits<PatchTile0>(L.d) ? launch_conv_patch<PatchTile0>(h, id, L, p, st) : launch_conv_patch<PatchTile2>(h, id, L, p, st);
}

int launch_patchp(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    return patchp_fits<PatchTile0>(L.d) ? launch_conv_patchp<PatchTile0>(h, id, L, p, st) : launch_conv_patchp<PatchTile2>(h, id, L, p, st);
}

// The grouped 3x3 kernel (mpx_gconv.h, tile id 16): one wave per 16 output pixels x channel block, GCONV_WAVES blocks per workgroup.  The
// grid is not capped: ceil(M / 16) <= 2^27 workgroups in x, the block quads in y.
bool gconv_accepts(const ConvLayer& L) {
    const int cg = L.groups > 1 ? L.d.cin / L.groups : 0, cb = gconv_cb(cg);
    return !(L.groups <= 1 || L.d.ksize != 3 || L.d.pad != 1 || (L.d.stride != 1 && L.d.stride != 2) || L.d.cin != L.d.cout || L.d.cin % L.groups ||
             (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) || L.d.cin % (cb * GCONV_WAVES) || L.d.k_packed != gconv_kp(cb) || L.cin_pad != L.d.cin ||
             L.cout_store != L.d.cout);
}

int launch_gconv(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    const int cg = L.groups > 1 ? L.d.cin / L.groups : 0, cb = gconv_cb(cg);
    // (a layer in mpx_gconvw.h's form has tile 16's planes only where a channel block is one group of 16: cg = 16)
    if (!gconv_accepts(L) || (L.gw && cg != 16))
        return fail(h, MPX_E_INTERNAL, "grouped conv: %s is not a 3x3 pad-1 layer of 4, 8, 16, 32 or 64 channels per group", L.d.name);
    if (p.r_hi || p.y_f32 || p.k1) return fail(h, MPX_E_ARG, "grouped conv: %s takes no residual operand and no fp32 output", L.d.name);
    p.n_tiles_c = L.d.cin / cb;
    const dim3 grid((unsigned)(((long long)p.M + 15) / 16), (unsigned)(p.n_tiles_c / GCONV_WAVES)), block(64 * GCONV_WAVES);
    switch (cb) {
        case 16: hipLaunchKernelGGL(gconv3x3_f16x3_kernel<16>, grid, block, 0, st, p); break;
        case 32: hipLaunchKernelGGL(gconv3x3_f16x3_kernel<32>, grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL(gconv3x3_f16x3_kernel<64>, grid, block, 0, st, p); break;
    }
    return launched(h, id);
}

// The grouped 3x3 kernel for any group count (mpx_gconvw.h, tile id 18): one wave per GCONVW_NT tiles of 16 output pixels x group x chunk of row
// fragments, GCONVW_WAVES units per workgroup.  The grid is not capped: ceil(M / (16 GCONVW_NT)) < 2^27 workgroups in x, the unit quads in y.
bool gconvw_accepts(const ConvLayer& L) {
    const int cg = L.groups > 1 ? L.d.cin / L.groups : 0;
    return L.gw && L.groups > 1 && L.d.ksize == 3 && L.d.pad == 1 && (L.d.stride == 1 || L.d.stride == 2) && L.d.cin == L.d.cout && L.d.cin % L.groups == 0 &&
           (cg == 16 || cg == 24 || cg == 48 || cg == 56 || cg == 120) && L.d.k_packed == gconvw_kp(cg) && L.d.cout_pad == L.groups * gconvw_rf(cg) * 16 &&
           L.cin_pad >= L.d.cin && L.cin_pad % 8 == 0 && L.cout_store >= L.d.cout && L.cout_store % 8 == 0 && !L.x_pitch && !L.y_pitch;
}

// the launch itself: width -> width in `groups` groups of 16, 24, 48, 56 or 120 channels (the callers check), p complete but for the two fields below
void gconvw_launch(int width, int groups, ConvParams& p, hipStream_t st) {
    const int cg = width / groups;
    p.n_tiles_c = groups;
    p.k_per_tap = width;        // the layer's width: where the output's pad channels begin
    const int units = groups * gconvw_nch(cg);
    const int per_wg = 16 * GCONVW_NT;
    const dim3 grid((unsigned)(((long long)p.M + per_wg - 1) / per_wg), (unsigned)((units + GCONVW_WAVES - 1) / GCONVW_WAVES)), block(64 * GCONVW_WAVES);
    switch (cg) {
        case 16: hipLaunchKernelGGL((gconvw3x3_f16x3_kernel<16, GCONVW_NT>), grid, block, 0, st, p); break;
        case 24: hipLaunchKernelGGL((gconvw3x3_f16x3_kernel<24, GCONVW_NT>), grid, block, 0, st, p); break;
        case 48: hipLaunchKernelGGL((gconvw3x3_f16x3_kernel<48, GCONVW_NT>), grid, block, 0, st, p); break;
        case 56: hipLaunchKernelGGL((gconvw3x3_f16x3_kernel<56, GCONVW_NT>), grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL((gconvw3x3_f16x3_kernel<120, GCONVW_NT>), grid, block, 0, st, p); break;
    }
}

int launch_gconvw(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    if (!gconvw_accepts(L))
        return fail(h, MPX_E_INTERNAL, "grouped conv: %s is not a 3x3 pad-1 layer of 16, 24, 48, 56 or 120 channels per group in the any-width form", L.d.name);
    if (p.r_hi || p.y_f32 || p.k1) return fail(h, MPX_E_ARG, "grouped conv: %s takes no residual operand and no fp32 output", L.d.name);
    gconvw_launch(L.d.cin, L.groups, p, st);
    return launched(h, id);
}

struct TileRow {
    int id;
    LaunchFn launch;
    bool (*eligible)(const mpx_conv_desc&);     // nullptr: every layer (tile 16: every GROUPED layer -- a layer is grouped by ConvLayer::groups, not by its descriptor: eligible())
    const char* refusal;                        // why mpx_set_conv_tile refuses a layer that is not eligible
    int dual;       // the tile whose DUAL kernel (launch_conv_tile<Cfg, true>) runs the layer fused with its downsample conv; -1: none
    bool split;     // the images behind the last whole round of tiles go to tile 2 (launch_conv)
};

// The product tile ids: every id default_tile hands out (include/mpx.h, mpx_set_conv_tile).
const TileRow kTiles[] = {
    {0, launch_conv_tile<ConvTile0>, nullptr, nullptr, -1, false},
    {1, launch_conv_tile<ConvTile1>, nullptr, nullptr, -1, false},
    {2, launch_conv_tile<ConvTile2, true>, nullptr, nullptr, 2, false},
    {4, launch_conv_tile<ConvTile4>, nullptr, nullptr, -1, false},
    {6, launch_patch, patch_eligible, "the patch kernel needs a 3x3 stride-1 layer whose input patch fits the LDS", -1, false},
    {7, launch_conv_tile<ConvTile7, true>, nullptr, nullptr, 7, false},
    {9, launch_conv256, conv256_eligible, "the 256x256 kernel runs 1x1 stride-1 layers with cout % 256 == 0 and cin % 64 == 0", -1, true},
    {10, launch_convx, convx_eligible,
     "the persistent expanding-1x1 kernel runs 1x1 stride-1 layers with cout % 256 == 0 and cin % 64 == 0, cin >= 128", 7, false},
    {12, launch_patchp, patchp_eligible,
     "the persistent patch kernel needs a 3x3 stride-1 layer with cout >= 128 and no residual operand whose input patch fits the LDS", -1, false},
    {13, launch_conv256p, conv256p_eligible,
     "the persistent 256x256 kernel runs 1x1 stride-1 layers with cout % 256 == 0, cin % 64 == 0 and no residual operand", -1, true},
    {14, launch_convw, convw_eligible,
     "the weights-in-registers expanding-1x1 kernel runs 1x1 stride-1 layers with cout % 256 == 0 and cin = 256", 7, false},
    {kGconvTile, launch_gconv, nullptr, "the grouped 3x3 kernel runs grouped layers (a ResNeXt block's conv2) and nothing else", -1, false},
    {kGconvwTile, launch_gconvw, nullptr,
     "the any-width grouped 3x3 kernel runs grouped layers of 16, 24, 48, 56 or 120 channels per group (a RegNetX / RegNetY block's f.b) and nothing else", -1, false},
};

// Dynamic LDS ceiling of every conv kernel (mpx_create): the kernels of kTiles with their DUAL forms, the stem + pool kernel, the block
// tails; the patch kernels size their LDS per layer.
struct KernelLds {
    const void* kernel;
    int bytes;
};
const KernelLds kKernelLds[] = {
    {(const void*)conv_f16x3_kernel<ConvTile0>, ConvTile0::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile1>, ConvTile1::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile1, false, true>, ConvTile1::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile2>, ConvTile2::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile7>, ConvTile7::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile2, true>, ConvTile2::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile7, true>, ConvTile7::LDS},
    {(const void*)conv256_f16x3_kernel, Conv256::LDS},
    {(const void*)convx_f16x3_kernel, ConvX::LDS},
    {(const void*)convw_f16x3_kernel<ConvW::K, true>, ConvW::LDS},
    {(const void*)conv256p_f16x3_kernel<false>, Conv256P::LDS},
    {(const void*)conv256p_f16x3_kernel<true>, Conv256P::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile4>, ConvTile4::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile0, false, false, true>, ConvTile0::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile1, false, false, true>, ConvTile1::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile2, false, false, true>, ConvTile2::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile4, false, false, true>, ConvTile4::LDS},
    {(const void*)conv_f16x3_kernel<ConvTile7, false, false, true>, ConvTile7::LDS},
    {(const void*)conv_f16x3_kernel<ConvGelu<ConvTile0>>, ConvTile0::LDS},
    {(const void*)conv_f16x3_kernel<ConvGelu<ConvTile1>>, ConvTile1::LDS},
    {(const void*)conv_f16x3_kernel<ConvGelu<ConvTile2>>, ConvTile2::LDS},
    {(const void*)conv_f16x3_kernel<ConvGelu<ConvTile4>>, ConvTile4::LDS},
    {(const void*)conv_f16x3_kernel<ConvGelu<ConvTile7>>, ConvTile7::LDS},
    {(const void*)attention_f16x3_kernel, (int)((size_t)2 * AT_HD * (AT_MAX_T + 8) * 2)},
    {(const void*)btail_f16x3_kernel<BtResC64>, BtResC64::LDS},
    {(const void*)btail_f16x3_kernel<BtResC128>, BtResC128::LDS},
    {(const void*)btail_f16x3_kernel<BtDualC64>, BtDualC64::LDS},
    {(const void*)btail_f16x3_kernel<BtHeadC64>, BtHeadC64::LDS},
    {(const void*)btail_f16x3_kernel<BtPw128>, BtPw128::LDS},
    {(const void*)conv3x3p_f16x3_kernel<PatchTile0>, kLdsLimit},
    {(const void*)conv3x3p_f16x3_kernel<PatchTile1>, kLdsLimit},
    {(const void*)conv3x3p_f16x3_kernel<PatchTile2>, kLdsLimit},
    {(const void*)conv3x3pp_f16x3_kernel<PatchTile0>, kLdsLimit},
    {(const void*)conv3x3pp_f16x3_kernel<PatchTile2>, kLdsLimit},
};

const TileRow* find_tile(int id) {
    for (const TileRow& r : kTiles)
        if (r.id == id) return &r;
    return nullptr;
}

// Layer L may run row r's kernel.  The predicates see the descriptor, whose cin is the channels per input pixel except in the small
// networks' planes, padded to 32 (cin_pad); the stem and the fc read planes of their own.  Only the generic kernel has a SLICE form, so an
// output-slice layer (y_pitch) runs the rows without a predicate -- tiles 0, 1, 2, 4 and 7 -- and nothing else.  An INPUT-slice layer (x_pitch: pixels
// farther apart than its K per tap) does the same: the generic kernel addresses a tap through pix_stride and walks k_per_tap within it, while
// the 256-row kernels (mpx_conv256.h, mpx_conv256p.h, mpx_convx.h, mpx_convw.h) and the patch kernels (cin = k_per_tap is their row pitch)
// read dense pixel rows.
bool eligible(const TileRow& r, const ConvLayer& L) {
    // a RegNetX grouped layer runs tile 18, and tile 16 where its shape is one of tile 16's (cg = 16, width % 64 == 0, pitch = width); tile 18 nothing else
    if (L.gw || r.id == kGconvwTile) return L.gw && ((r.id == kGconvwTile && gconvw_accepts(L)) || (r.id == kGconvTile && gconv_accepts(L) && L.d.cin / L.groups == 16));
    if (L.groups > 1 || r.id == kGconvTile) return L.groups > 1 && r.id == kGconvTile;     // a grouped layer runs tile 16, and tile 16 nothing else
    if (L.epi_act && r.eligible) return false;      // only the generic kernel's epilogue has an activation other than ReLU (ConvGelu)
    return !r.eligible || (!L.is_fc && !L.is_stem && L.cin_pad == L.d.cin && !L.y_pitch && !L.x_pitch && r.eligible(L.d));
}

int launch_tile(mpx_engine* h, int id, const ConvLayer& L, ConvParams& p, hipStream_t st) {
    const TileRow* r = find_tile(id);
    if (!r) return fail(h, MPX_E_INTERNAL, "conv: no kernel for tile id %d", id);
    return r->launch(h, id, L, p, st);
}

// Default variant per layer, from tools/tile_sweep.sh and in-network tools/layer_profile.py runs on MI355X at
// batch 2048: cout <= 64 layers take a 64-row tile (no zero-padded MFMA rows); of the rest, the 128x128 tile
// with two workgroups per CU wins on every 1x1 shape by 5-15 % (one workgroup's HBM-bound epilogue overlaps the
// other's K loop) and wide 3x3 layers keep the 128x256 tile (fewest L2 bytes per FLOP; 7 % faster in the
// network although the isolated layer bench prefers 128x128); the stride-1 ones whose input patch fits the LDS run
// the patch kernel (mpx_conv3p.h, tile id 6).  Every tile stays selectable.
int default_tile(const mpx_conv_desc& d) {
    if (d.cout <= 64) return d.ksize >= 3 ? 1 : 4;       // (the patch kernel is 10 % slower than tile 1 on 64->64 in the network)
    // ... as one persistent workgroup per CU (mpx_conv3pp.h) where the layer has no residual operand: in the network (batch 2340,
    // A/B in one call) 128->128 on 28x28 3.89 -> 3.67 ms, 256->256 on 14x14 24.65 -> 24.49 ms per batch; 7x7 maps lose 1 % (2.29 -> 2.32)
#ifndef MPX_PROBE_NO_PERSISTENT_PATCH   // A/B builds only (tools/ab_lib.sh)
    // ... and on AlexNet's 13x13 maps (the only maps between 7 and 14 in any network here) where the cout tiles are a power of two, so that
    // the persistent grid fills every CU: in the network at batch 2340, on two boxes, 384->256 1.344 -> 1.285 / 1.404 -> 1.383 ms, 256->256
    // 0.931 -> 0.873 / 0.978 -> 0.945.  192->384 is three cout tiles, a grid of 240 of the 256 CUs: 1.118 -> 1.084 on one box, 1.158 -> 1.184
    // on the other, so it keeps tile 6.  (Under three rounds of tiles the persistent form loses: 4-7 % at batch 512, 0-3 % at 1024.)
    if (patchp_eligible(d) && (d.hout >= 14 || (d.hout == 13 && ((d.cout / 128) & (d.cout / 128 - 1)) == 0))) return 12;
#endif
    if (patch_eligible(d)) return 6;                      // 3x3 stride 1 on 28x28 / 14x14 / 7x7 maps: -10..18 % against tile 0
    if (d.ksize == 3) return 0;
    // AlexNet's two layers with kernel sizes no other network here has (tools/layer_profile.py alexnet B with MPX_TILE_SWEEP=1, in the
    // network).  5x5 64->192: three 64-row cout tiles instead of two 128-row ones a quarter of whose MFMA rows are padding -- tile 7 -> 1
    // 2.915 -> 2.703 ms at batch 2340, 1.280 -> 1.188 at 1024, 0.662 -> 0.622 at 512.  classifier.1 (6x6 valid conv, K = 9216): long K, so the
    // four waves per SIMD of tile 7 cover nothing -- tile 7 -> 2 0.551 -> 0.544 ms at 2340, 0.268 -> 0.263 at 1024, a tie at 512
    if (d.ksize == 5 && d.cout % 128 != 0 && d.cout % 64 == 0) return 1;
    if (d.ksize == 6) return 2;
    // expanding 1x1 layers (short K, long epilogue): four waves per SIMD cover the epilogue better, -2..4 % in the
    // network; the reducing ones (long K) gain nothing from it
    // ... and on 28x28 / 14x14 maps with K >= 128 the persistent pipelined kernel (mpx_convx.h) is 2-4 % faster still in the
    // network (256->1024: 21.5 -> 21.0 ms, 128->512: 6.5 -> 6.2); on 7x7 maps and K = 64 it ties tile 7
    // ... and with K = 256 exactly (256 -> 1024, a fifth of ResNet-101's conv time) the kernel that keeps the weights of a wave in its
    // 256 AGPRs and only pixels in the LDS (mpx_convw.h): in the network at batch 2340, A/B in one call, 24.3 -> 21.3 ms for the 23 layers
#ifndef MPX_PROBE_NO_CONVW               // A/B builds only (tools/ab_lib.sh)
    if (convw_eligible(d) && d.cout > d.cin && d.hout >= 14) return 14;
#endif
    // (round 4: on 7x7 maps too -- 512 -> 2048 x3 3.53 -> 3.38 ms per batch in the network, A/B in one call; round 2 had measured a tie)
    if (convx_eligible(d) && d.cout > d.cin) return 10;
    if (d.stride == 1 && d.cout > d.cin) return 7;
    // reducing / square 1x1 stride-1 layers with cout % 256 == 0: the 256x256 tile (mpx_conv256.h) halves the operand bytes
    // per MAC and runs +10..18 % (1024->256: 365 vs 322 TFLOP/s, 1024->512: 411 vs 346); expanding layers lose on it (one
    // workgroup per CU: nothing covers the long epilogue)
    // ... as one persistent workgroup per CU with a register epilogue (mpx_conv256p.h) where the layer has no residual operand (all of
    // them in the torchvision ResNets): in the network at batch 2340, A/B in one call, 1024->256 13.73 -> 13.12 ms, 512->256 1.47 -> 1.32,
    // 1024->512 1.18 -> 1.11, 2048->512 1.11 -> 1.10 per batch
#ifdef MPX_PROBE_NO_PERSISTENT_256      // A/B builds only (tools/ab_lib.sh)
    if (conv256_eligible(d)) return 9;
#endif
    if (conv256_eligible(d)) return conv256p_eligible(d) ? 13 : 9;
    return 2;
}

}  // namespace

#include "mpx_plan.h"

namespace {

// The ConvParams of layer L over B images: its packed weights, the input planes in_* (the ImageNet stem: the engine's padded NHWC4 staging,
// where a (ky) tap is one 64-B run of 8 pixels x 4 channels, no bounds to check), the output planes y_*.  The output pixels must fit
// 32-bit indices; the callers check the extent of the input planes their kernel indexes.
int conv_params(mpx_engine* h, const ConvLayer& L, const half_t* in_hi, const half_t* in_lo, half_t* y_hi, half_t* y_lo, int B, ConvParams& p) {
    std::memset(&p, 0, sizeof p);
    p.w_hi = L.w_hi; p.w_lo = L.w_lo; p.scale = L.scale; p.shift = L.shift;
    p.y_hi = y_hi; p.y_lo = y_lo;
    p.cout = L.cout_store;
    p.relu = L.d.relu;
    p.ktot = L.d.k_packed;
    if (L.is_stem) {
        // a K step is one kernel row: a run of 8 pixels x 4 channels starting at the window's left edge in the staging, whose
        // 3-pixel border already holds the padding (the 7x7 stem's pad 3: origin shift 0; the VGG 3x3 pad-1 layer: -2).  A run that
        // passes a row's end reads the next row of the same image (row 2y + 3 + ky <= 229 for the stem, y + 2 + ky <= 227 for VGG),
        // and meets the zero weights of px >= ksize.  SqueezeNet's unpadded 3x3 stride-2 stem: origin shift +3, rows 2y + 3 + ky <= 225,
        // columns 2x + 3 .. 2x + 10 <= 230 -- the last column's run passes the row end by ONE pixel (the first of the next row, always inside
        // the image's own 230 x 230 staging since the row is at most 225) and meets zero weights there.  AlexNet's 11-wide row is two K steps, a run of 16 pixels (k_per_tap = 64; the
        // kernel walks c0 = 0, 32 within a tap): origin shift -1, columns 4x + 1 .. 4x + 16 <= 232, rows 4y + 1 + ky <= 227.
        p.x_hi = h->in_hi; p.x_lo = h->in_lo;
        p.hin = MPX_IMG_PAD; p.win = MPX_IMG_PAD; p.pix_stride = 4;
        p.kh = L.d.ksize; p.kw = 1; p.stride = L.d.stride; p.pad = L.d.pad - (MPX_IMG_PAD - MPX_IMG) / 2; p.k_per_tap = L.d.k_packed / L.d.ksize;
    } else {
        // an input-slice layer (x_pitch) gets the BASE of the planes it reads a channel range of, as an output-slice layer the base of y.
        // The kernel builds its buffer descriptor from the advanced pointer with hin * win * pix_stride records per image, so the descriptor
        // spans x_offset elements past the end of the planes: no load goes there (a pixel's offsets stay below k_per_tap = the slice's width,
        // so the last pixel's read ENDS at the end of the planes), but the descriptor's out-of-range zeroing no longer guards that tail.
        p.x_hi = in_hi ? in_hi + L.x_offset : in_hi; p.x_lo = in_lo ? in_lo + L.x_offset : in_lo;
        p.hin = L.d.hin; p.win = L.d.hin; p.pix_stride = L.x_pitch ? L.x_pitch : L.cin_pad;
        p.kh = L.d.ksize; p.kw = L.d.ksize; p.stride = L.d.stride; p.pad = L.d.pad; p.k_per_tap = L.cin_pad;
    }
    p.ho = L.d.hout; p.wo = L.d.hout;
    if (L.rows > 0) {       // a token layer (ViT): `rows` rows per image that are no square map -- a column of rows x 1 pixels
        p.hin = L.rows; p.win = 1;
        p.ho = L.rows; p.wo = 1;
    }
    const long long M = (long long)B * p.ho * p.wo;
    if (M > 0x7fffffffLL) return fail(h, MPX_E_ARG, "batch too large for 32-bit pixel indices");
    p.M = (int)M;
#ifdef MPX_DIAG
    p.stamps = h->stamps;
#endif
    return 0;
}

int launch_conv(mpx_engine* h, int i, const half_t* in_hi, const half_t* in_lo, const half_t* r_hi,
                const half_t* r_lo, half_t* y_hi, half_t* y_lo, float* y_f32, int B, hipStream_t st) {
    const ConvLayer& L = h->convs[i];
    if (!L.loaded) return fail(h, MPX_E_STATE, "layer %d (%s) has no weights", i, L.d.name);
    ConvParams p;
    if (int rc = conv_params(h, L, in_hi, in_lo, y_hi, y_lo, B, p)) return rc;
    if ((long long)B * p.hin * p.win > 0x7fffffffLL) return fail(h, MPX_E_ARG, "batch too large for 32-bit pixel indices");
    p.r_hi = r_hi; p.r_lo = r_lo; p.y_f32 = y_f32;
    if (L.y_pitch) {        // output slice: y_* is the base of the concatenated planes; the kernel gets it advanced to the layer's first channel
        if (r_hi || r_lo || y_f32) return fail(h, MPX_E_ARG, "conv: %s writes a channel slice; it takes no residual operand and no fp32 output", L.d.name);
        p.y_pitch = L.y_pitch;
        p.y_hi += L.y_offset; p.y_lo += L.y_offset;
    }
    ProfScope ps(h, st, OP_CONV, i);
    h->last_kernels = 0;
    // The 256x256 kernel keeps ONE workgroup per CU, so a launch runs in "rounds" of num_cus tiles and a small remainder would
    // keep most CUs idle for a whole tile time (14x14 maps at batch 2048: 1568 tiles = 6.125 rounds).  Then the images of
    // the whole rounds go to that kernel and the last few images (images are independent: an image range is a pointer
    // offset) to the 128x128 kernel, whose tiles are a quarter of the size and which sums in the same order (bit-identical
    // scores wherever a mask sits in the batch): 1024->256 12.9 -> 12.3 ms, 2048->512 1.15 -> 1.01 ms per batch.  (The same
    // split of the 3x3 patch kernel's and tile 0's last round was measured and gains nothing: their remainder lives as long
    // as one of their tiles whatever its tile size)
    const TileRow* row = find_tile(L.tile);
    if (row && row->split && !L.is_stem && !L.y_pitch) {     // (eligible() keeps slice layers off these rows; the split's offsets assume pitch = cout)
        const long long M = p.M, tiles_c = (p.cout + Conv256::TC - 1) / Conv256::TC, tiles_p = (M + Conv256::TP - 1) / Conv256::TP;
        const long long total = tiles_p * tiles_c, rounds = total / h->num_cus, rest = total - rounds * h->num_cus;
        const long long howo = (long long)p.ho * p.wo;
        const long long n_a = rounds * h->num_cus / tiles_c * Conv256::TP / howo;      // images that fill the whole rounds
        if (rounds >= 1 && rest > 0 && 2 * rest <= h->num_cus && n_a >= 1 && n_a < B) {
            ConvParams q = p;
            p.M = (int)(n_a * howo);
            int rc = launch_tile(h, L.tile, L, p, st);
            if (rc) return rc;
            const size_t xo = (size_t)n_a * p.hin * p.win * p.pix_stride, yo = (size_t)n_a * howo * p.cout;
            q.M = (int)(M - n_a * howo);
            q.x_hi += xo; q.x_lo += xo;
            q.y_hi += yo; q.y_lo += yo;
            if (q.r_hi) { q.r_hi += yo; q.r_lo += yo; }
            return launch_tile(h, 2, L, q, st);
        }
    }
    return launch_tile(h, L.tile, L, p, st);
}

// A block's last 1x1 conv with its downsample branch K-concatenated: out = relu(s * (W3' . t2 + Wds' . x) + shift)
// (build_fused).  in = t2 planes [B][ho][wo][k1], x2 = block input planes [B][hin2][hin2][k2].
int launch_conv_fused(mpx_engine* h, int i, const half_t* in_hi, const half_t* in_lo, const half_t* x2_hi,
                      const half_t* x2_lo, half_t* y_hi, half_t* y_lo, int B, hipStream_t st) {
    const ConvLayer& L = h->convs[i];
    if (!L.fuse_main || !L.fused_loaded) return fail(h, MPX_E_STATE, "layer %d (%s) has no fused weights", i, L.d.name);
    const ConvLayer& D = h->convs[L.fuse_partner];
    ConvParams p;
    if (int rc = conv_params(h, L, in_hi, in_lo, y_hi, y_lo, B, p)) return rc;
    if ((long long)B * D.d.hin * D.d.hin > 0x7fffffffLL) return fail(h, MPX_E_ARG, "batch too large for 32-bit pixel indices");
    p.w_hi = L.fw_hi; p.w_lo = L.fw_lo; p.scale = L.fscale; p.shift = L.fshift;
    p.k1 = L.d.cin; p.ktot = L.d.cin + D.d.cin;
    p.x2_hi = x2_hi; p.x2_lo = x2_lo;
    p.hin2 = D.d.hin; p.win2 = D.d.hin; p.pix_stride2 = D.d.cin; p.stride2 = D.d.stride;
    ProfScope ps(h, st, OP_CONV, i);
    h->last_kernels = 0;
    const TileRow* row = find_tile(L.tile);
    // Bottleneck stages' first conv3 + downsample (the main layer on one of the 256-row tiles 9, 10, 13, 14, whose rows send a fused launch to
    // tile 7): the DUAL form of the persistent 256x256 kernel (mpx_conv256p.h), reported as tile 13.  In the network at batch 2340, parent
    // build and this one alternating twice in one call (tile 7's dual kernel -> this one, ms per batch): layer2.0 (K = 128 + 256, 28x28)
    // 2.549 / 2.535 -> 2.107 / 2.089, layer3.0 (256 + 512, 14x14) 2.120 / 2.116 -> 1.758 / 1.743, layer4.0 (512 + 1024, 7x7) 1.869 / 1.879 ->
    // 1.593 / 1.583: every stage gains 15-17 %, so eligibility is the whole rule.  A last round that is not whole ends the persistent
    // walk raggedly: splitting it off to tile 2's dual kernel (as launch_conv does for the plain 256x256 tile) was measured and loses or
    // ties -- batch 2048, ragged / split, two runs each: layer3.0 (24.5 rounds) 1.512 1.505 / 1.532 1.541 ms, layer4.0 (12.25 rounds) 1.397
    // 1.380 / 1.375 1.382 -- and was not kept (profiles/dual256p_ab.txt).
    // mpx_set_conv_tile(i, 7) or (i, 2) on the main layer still forces the generic dual kernels; BasicBlock fusions (3x3 main conv) are
    // not eligible and keep them too.
#ifndef MPX_PROBE_NO_DUAL256P            // A/B builds only (tools/ab_lib.sh)
    if ((L.tile == 9 || L.tile == 10 || L.tile == 13 || L.tile == 14) && conv256p_dual_eligible(L, D)) {
        const int rc = launch_conv256p_dual(h, L, p, st);
        if (rc != 0) return rc < 0 ? rc : 0;
    }
#endif
    return launch_tile(h, row && row->dual >= 0 ? row->dual : 7, L, p, st);     // (mpx_conv_dual_bn_act on any other tile: tile 7's)
}

// The ImageNet stem (7x7 stride-2 conv + BN + ReLU) with its 3x3 stride-2 pad-1 max pool in ONE launch (mpx_conv.h, POOL): writes the
// pooled planes [B][56][56][64]; the 112x112 conv output is never stored.  Needs the 64-row tile 1 (the stem's default).
bool stem_pool_eligible(const mpx_engine* h) {
    if (h->small || h->googlenet || h->convs.empty()) return false;     // (GoogLeNet's stem has the shape, but a ceil-mode unpadded pool behind it)
    const ConvLayer& L = h->convs[0];
    return L.is_stem && L.d.cout == 64 && L.d.hout == 112 && (L.d.hout / 2) % POOL_PY == 0 && (L.d.hout / 2) % POOL_PX == 0 && L.d.relu;
}

int launch_stem_pool(mpx_engine* h, half_t* y_hi, half_t* y_lo, int B, hipStream_t st) {
    const ConvLayer& L = h->convs[0];
    if (!stem_pool_eligible(h)) return fail(h, MPX_E_STATE, "stem + max pool: this architecture has no 7x7 stem with a max pool");
    if (!L.loaded) return fail(h, MPX_E_STATE, "layer 0 (%s) has no weights", L.d.name);
    ConvParams p;
    if (int rc = conv_params(h, L, nullptr, nullptr, y_hi, y_lo, B, p)) return rc;
    p.n_tiles_c = 1;
    const long long nblocks = (long long)B * (p.ho / 2 / POOL_PY) * (p.wo / 2 / POOL_PX);
    if (nblocks > 0x7fffffffLL) return fail(h, MPX_E_ARG, "conv grid out of range");
    ProfScope ps(h, st, OP_CONV, 0);
    hipLaunchKernelGGL((conv_f16x3_kernel<ConvTile1, false, true>), dim3((unsigned)nblocks), dim3(ConvTile1::NT), ConvTile1::LDS, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// K permutation of a block tail's conv3 operand (mpx_btail.h): K position 8g + j of a 32-wide step holds channel (j>>2)*16 + 4g + (j&3),
// because that is where the conv2 accumulators of a lane group g sit (D layout of v_mfma_f32_16x16x32_f16: registers 4g .. 4g+3 of
// two stacked 16-row fragments).
constexpr int bt_perm_channel(int kpos) {
    const int s = kpos >> 5, q = kpos & 31, g = q >> 3, j = q & 7;
    return 32 * s + (j >> 2) * 16 + 4 * g + (j & 3);
}
constexpr bool bt_perm_is_bijection() {        // every channel of [0,64) exactly once, each 32-wide K step onto its own 32 channels
    bool seen[BT_MID] = {};
    for (int k = 0; k < BT_MID; ++k) {
        const int c = bt_perm_channel(k);
        if (c < 0 || c >= BT_MID || seen[c] || (c >> 5) != (k >> 5)) return false;
        seen[c] = true;
    }
    return true;
}
static_assert(bt_perm_is_bijection(), "K permutation of the block tail's conv3 operand");
static_assert(bt_perm_channel(0) == 0 && bt_perm_channel(3) == 3 && bt_perm_channel(4) == 16 && bt_perm_channel(8) == 4 && bt_perm_channel(36) == 48,
              "K position 8g + j <-> channel (j>>2)*16 + 4g + (j&3): registers 4g..4g+3 of two stacked 16-row accumulator fragments");

// Upload the K-permuted copy of packed planes `hi`/`lo` ([rows >= 256][K], piece-major, host) into the tail's own planes:
// columns [0,64) permuted, columns [64,K) (the downsample branch of a DUAL tail) as they are.
int upload_tail_planes(mpx_engine* h, TailBlock& tb, const std::vector<uint16_t>& hi, const std::vector<uint16_t>& lo, int K) {
    std::vector<uint16_t> ph((size_t)BT_OUT * K), pl((size_t)BT_OUT * K);
    for (int row = 0; row < BT_OUT; ++row)
        for (int k = 0; k < K; ++k) {
            const int src = k < BT_MID ? bt_perm_channel(k) : k;
            ph[w_packed_index(row, k, K)] = hi[w_packed_index(row, src, K)];
            pl[w_packed_index(row, k, K)] = lo[w_packed_index(row, src, K)];
        }
    MPX_HIP(h, hipMemcpy(tb.w3p_hi, ph.data(), ph.size() * 2, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(tb.w3p_lo, pl.data(), pl.size() * 2, hipMemcpyHostToDevice));
    tb.ready = true;
    return 0;
}

TailBlock* tail_of_conv3(mpx_engine* h, int c3) {
    for (TailBlock& tb : h->tails)
        if (tb.c3 == c3) return &tb;
    return nullptr;
}

bool tails_ready(const mpx_engine* h) {
    if (h->tails.empty()) return false;
    for (const TailBlock& tb : h->tails)
        if (!tb.ready || !h->convs[tb.c2].loaded || !h->convs[tb.next1].loaded || !h->convs[tb.c1].loaded) return false;
    return true;
}

// One block tail (mpx_btail.h): t1 planes [B][56][56][64], x = identity planes [B][56][56][256] (first block of layer1: the block
// input [B][56][56][64]), y = block output [B][56][56][256], z = the next block's conv1 output [B][56][56][64 | 128].
int launch_btail(mpx_engine* h, int ti, const half_t* t_hi, const half_t* t_lo, const half_t* x_hi, const half_t* x_lo,
                 half_t* y_hi, half_t* y_lo, half_t* z_hi, half_t* z_lo, int B, hipStream_t st) {
    const TailBlock& tb = h->tails[ti];
    const ConvLayer& L2 = h->convs[tb.c2];
    const ConvLayer& L3 = h->convs[tb.c3];
    const ConvLayer& N1 = h->convs[tb.next1];
    if (!tb.ready || !L2.loaded || !N1.loaded) return fail(h, MPX_E_STATE, "block tail %s: weights missing", L2.d.name);
    const bool dual = tb.ds >= 0;
    const bool head = t_hi == nullptr;          // the block's own conv1 runs inside the launch, on the patch of the block input
    if (head && !dual) return fail(h, MPX_E_ARG, "block tail %s: only a block with a downsample branch (64-channel input) can run its own conv1 in the launch", L2.d.name);
    BtParams p;
    std::memset(&p, 0, sizeof p);
    p.t_hi = head ? x_hi : t_hi; p.t_lo = head ? x_lo : t_lo;
    if (head) {
        const ConvLayer& L1 = h->convs[tb.c1];
        if (!L1.loaded) return fail(h, MPX_E_STATE, "block tail %s: weights of %s missing", L2.d.name, L1.d.name);
        if (!(L1.d.cin == BT_MID && L1.d.cout == BT_MID && L1.d.ksize == 1 && L1.d.stride == 1)) return fail(h, MPX_E_INTERNAL, "block tail: %s is not a 64 -> 64 1x1 conv", L1.d.name);
        p.w0_hi = L1.w_hi; p.w0_lo = L1.w_lo; p.sc0 = L1.scale; p.sh0 = L1.shift;
    }
    p.w2_hi = L2.w_hi; p.w2_lo = L2.w_lo; p.sc2 = L2.scale; p.sh2 = L2.shift;
    p.w3_hi = tb.w3p_hi; p.w3_lo = tb.w3p_lo;
    p.sc3 = dual ? L3.fscale : L3.scale; p.sh3 = dual ? L3.fshift : L3.shift;
    p.r_hi = x_hi; p.r_lo = x_lo; p.y_hi = y_hi; p.y_lo = y_lo;
    p.w1_hi = N1.w_hi; p.w1_lo = N1.w_lo; p.sc1 = N1.scale; p.sh1 = N1.shift;
    p.z_hi = z_hi; p.z_lo = z_lo;
    p.B = B; p.H = L2.d.hin; p.W = L2.d.hin;
    if (p.H % BT_TY || p.W % BT_TX) return fail(h, MPX_E_INTERNAL, "block tail: %dx%d map is not a whole number of 8x14 tiles", p.H, p.W);
    p.tiles_x = p.W / BT_TX;
    p.tiles_per_img = (p.H / BT_TY) * p.tiles_x;
    const long long n_tiles = (long long)B * p.tiles_per_img;
    if (n_tiles <= 0 || n_tiles > 0x7fffffffLL) return fail(h, MPX_E_ARG, "block tail: batch out of range");
    p.n_tiles = (int)n_tiles;
#ifdef MPX_DIAG
    p.stamps = h->stamps;
#endif
    const long long resident = 2LL * h->num_cus;                       // two 80-KB workgroups per CU
    const unsigned grid = (unsigned)std::min<long long>(resident / 8 * 8, (n_tiles + 7) / 8 * 8);
    ProfScope ps(h, st, OP_CONV, tb.c2);
    if (head) hipLaunchKernelGGL(btail_f16x3_kernel<BtHeadC64>, dim3(grid), dim3(256), BtHeadC64::LDS, st, p);
    else if (dual) hipLaunchKernelGGL(btail_f16x3_kernel<BtDualC64>, dim3(grid), dim3(256), BtDualC64::LDS, st, p);
    else if (N1.d.cout == 128) hipLaunchKernelGGL(btail_f16x3_kernel<BtResC128>, dim3(grid), dim3(256), BtResC128::LDS, st, p);
    else hipLaunchKernelGGL(btail_f16x3_kernel<BtResC64>, dim3(grid), dim3(256), BtResC64::LDS, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// One pointwise tail (mpx_btail.h): t2 planes [M][128], x = identity planes [M][512], y = block output [M][512], z = the next block's
// conv1 output [M][128], M = B * H * W pixels in tiles of 128.  The weights are the packed planes of the two layers themselves.
int launch_ptail(mpx_engine* h, int ti, const half_t* t_hi, const half_t* t_lo, const half_t* x_hi, const half_t* x_lo,
                 half_t* y_hi, half_t* y_lo, half_t* z_hi, half_t* z_lo, int B, hipStream_t st) {
    const PointTail& pt = h->ptails[ti];
    const ConvLayer& L3 = h->convs[pt.c3];
    const ConvLayer& N1 = h->convs[pt.next1];
    if (!L3.loaded || !N1.loaded) return fail(h, MPX_E_STATE, "pointwise tail %s: weights missing", L3.d.name);
    if (L3.d.k_packed != BtPw128::MID || N1.d.k_packed != BtPw128::OUT) return fail(h, MPX_E_INTERNAL, "pointwise tail %s: packed K %d / %d", L3.d.name, L3.d.k_packed, N1.d.k_packed);
    BtParams p;
    std::memset(&p, 0, sizeof p);
    p.t_hi = t_hi; p.t_lo = t_lo;
    p.w3_hi = L3.w_hi; p.w3_lo = L3.w_lo; p.sc3 = L3.scale; p.sh3 = L3.shift;
    p.r_hi = x_hi; p.r_lo = x_lo; p.y_hi = y_hi; p.y_lo = y_lo;
    p.w1_hi = N1.w_hi; p.w1_lo = N1.w_lo; p.sc1 = N1.scale; p.sh1 = N1.shift;
    p.z_hi = z_hi; p.z_lo = z_lo;
    p.B = B; p.H = L3.d.hin; p.W = L3.d.hin;
    const long long M = (long long)B * p.H * p.W;
    const long long n_tiles = (M + BtPw128::TP - 1) / BtPw128::TP;
    if (n_tiles <= 0 || M > 0x7fffffffLL) return fail(h, MPX_E_ARG, "pointwise tail: batch out of range");
    p.n_tiles = (int)n_tiles;
    const long long resident = 2LL * h->num_cus;                       // two 72-KB workgroups per CU
    const unsigned grid = (unsigned)std::min<long long>(resident, n_tiles);
    ProfScope ps(h, st, OP_CONV, pt.c3);
    hipLaunchKernelGGL(btail_f16x3_kernel<BtPw128>, dim3(grid), dim3(256), BtPw128::LDS, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// Layers c3 and next1 of pointwise tail k run as its one launch: bit 2 of the fusion mask, and no tile override on either layer
bool ptail_in_use(const mpx_engine* h, int k) {
    const PointTail& pt = h->ptails[k];
    for (int li : {pt.c3, pt.next1})
        if (!h->convs[li].loaded || h->convs[li].tile != default_tile(h->convs[li].d)) return false;
    return true;
}

// Fused planes of a (main, ds) pair from the host copies of both layers.  With s3 = g3/sqrt(v3+eps) and sd likewise,
//   bn3(W3.t2) + bnd(Wd.x) = s * ((W3 * s3/s) . t2 + (Wd * sd/s) . x) + shift3 + shiftd,   s = max(|s3|, |sd|) per channel
// (both ratios are <= 1 in magnitude, so a vanishing gamma on either branch is harmless).  The scaled rows are rounded
// to fp32 once and then split into hi + lo like any other weight (22 bits); per-row power-of-two normalisation as
// mpx_pack_conv_weights.
int build_fused(mpx_engine* h, int main) {
    ConvLayer& L = h->convs[main];
    ConvLayer& D = h->convs[L.fuse_partner];
    const int cout = L.d.cout, k1 = L.d.cin, k2 = D.d.cin, K = k1 + k2, rows = L.d.cout_pad;
    std::vector<uint16_t> hi((size_t)rows * K, 0), lo((size_t)rows * K, 0);
    std::vector<float> sc(rows, 0.f), sh(rows, 0.f), row(K);
    for (int co = 0; co < cout; ++co) {
        const double s3 = (double)L.hgamma[co] / std::sqrt((double)L.hvar[co] + (double)L.heps);
        const double sd = (double)D.hgamma[co] / std::sqrt((double)D.hvar[co] + (double)D.heps);
        double s = std::fmax(std::fabs(s3), std::fabs(sd));
        if (!(s > 0.0) || !std::isfinite(s)) s = 1.0;
        const double r3 = s3 / s, rd = sd / s;
        float mx = 0.f;
        for (int k = 0; k < k1; ++k) { row[k] = (float)((double)L.hw[(size_t)co * k1 + k] * r3); mx = std::fmax(mx, std::fabs(row[k])); }
        for (int k = 0; k < k2; ++k) { row[k1 + k] = (float)((double)D.hw[(size_t)co * k2 + k] * rd); mx = std::fmax(mx, std::fabs(row[k1 + k])); }
        int e = 0;
        if (mx > 0.f && std::isfinite(mx)) {
            int ex;
            std::frexp(mx, &ex);
            e = 10 - ex;
        }
        for (int k = 0; k < K; ++k) {
            const float sv = std::ldexp(row[k], e);
            const half_t vh = (half_t)sv;
            const half_t vl = (half_t)(sv - (float)vh);
            hi[w_packed_index(co, k, K)] = half_bits(vh);
            lo[w_packed_index(co, k, K)] = half_bits(vl);
        }
        sc[co] = (float)std::ldexp(s, -e);
        sh[co] = (float)(((double)L.hbeta[co] - (double)L.hmean[co] * s3) + ((double)D.hbeta[co] - (double)D.hmean[co] * sd));
    }
    MPX_HIP(h, hipMemcpy(L.fw_hi, hi.data(), hi.size() * 2, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(L.fw_lo, lo.data(), lo.size() * 2, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(L.fscale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(L.fshift, sh.data(), sh.size() * 4, hipMemcpyHostToDevice));
    L.fused_loaded = true;
    // (the host copies of both layers stay: they are small, and reloading ONE layer of the pair later must rebuild these planes)
    if (TailBlock* tb = tail_of_conv3(h, main)) return upload_tail_planes(h, *tb, hi, lo, K);
    return 0;
}

// ---- kernel arguments of the ops beside the convs ---------------------------------------------------------------------------------
// One builder per *Params struct: the ONLY place that fills it and computes its derived fields (output side, pixel / row / unit counts,
// channel range).  A stand-alone entry checks its arguments and calls the builder with them; mpx_forward's case calls it with the layer
// record's fields.  The launchers below take the finished struct and the launch's profile tag (ProfTag() from a stand-alone entry).

template <class P>
P zeroed() {
    P p;
    std::memset(&p, 0, sizeof p);
    return p;
}

template <class P>
void set_planes(P& p, const void* x_hi, const void* x_lo, void* y_hi, void* y_lo) {
    p.x_hi = (const half_t*)x_hi; p.x_lo = (const half_t*)x_lo; p.y_hi = (half_t*)y_hi; p.y_lo = (half_t*)y_lo;
}

// true when one of the pointers is not 16-byte aligned (a null pointer is: an entry checks for those first, where it forbids them)
bool planes_misaligned(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if ((uintptr_t)q & 15) return true;
    return false;
}

// output side of a depthwise layer (padding (k - 1) / 2)
int dw_out_side(int hin, int stride) { return (hin - 1) / stride + 1; }

CatNormParams catnorm_params(const void* fresh_hi, const void* fresh_lo, int g, int fresh_stride, void* raw_hi, void* raw_lo, int c_total,
                             int c_old, const float* scale, const float* shift, void* out_hi, void* out_lo, int c_norm, long long npix) {
    CatNormParams p = zeroed<CatNormParams>();
    const bool norm = out_hi != nullptr;
    p.f_hi = (const half_t*)fresh_hi; p.f_lo = (const half_t*)fresh_lo;
    p.r_hi = (half_t*)raw_hi; p.r_lo = (half_t*)raw_lo;
    p.y_hi = (half_t*)out_hi; p.y_lo = (half_t*)out_lo;
    p.scale = scale; p.shift = shift;
    p.npix = npix; p.f_stride = fresh_stride; p.c_total = c_total; p.c_old = c_old;
    p.c_begin = norm ? 0 : c_old;
    p.c_end = norm ? c_norm : c_old + g;
    return p;
}

// every depthwise + BatchNorm form (DwForm below): clamp_in is the one-pixel ReLU6 form's, act_in / act_out the run form's with SiLU
DwParams dw_params(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, const float* w, const float* scale, const float* shift, int B,
                   int hin, int pitch, int stride, int clamp_in, int act_in, int act_out) {
    DwParams p = zeroed<DwParams>();
    set_planes(p, x_hi, x_lo, y_hi, y_lo);
    p.w = w; p.scale = scale; p.shift = shift;
    p.hin = hin; p.ho = dw_out_side(hin, stride); p.pitch = pitch; p.stride = stride; p.clamp_in = clamp_in != 0;
    p.act_in = act_in; p.act_out = act_out;
    p.rows = (long long)B * p.ho;
    p.npix = p.rows * p.ho;
    return p;
}

CnDwLnParams cn_dwln_params(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, const float* w, const float* bias, const float* gamma,
                            const float* beta, float eps, int B, int hin, int C) {
    CnDwLnParams p = zeroed<CnDwLnParams>();
    set_planes(p, x_hi, x_lo, y_hi, y_lo);
    p.w = w; p.bias = bias; p.gamma = gamma; p.beta = beta;
    p.H = hin; p.C = C; p.eps = eps;
    p.units = (long long)B * p.H * ((p.H + CN_DW_W - 1) / CN_DW_W);
    return p;
}

CnLnParams cn_ln_params(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, const float* gamma, const float* beta, float eps,
                        long long rows, long long in_stride, int C) {
    CnLnParams p = zeroed<CnLnParams>();
    set_planes(p, x_hi, x_lo, y_hi, y_lo);
    p.gamma = gamma; p.beta = beta; p.rows = rows; p.in_stride = in_stride; p.C = C; p.eps = eps;
    return p;
}

CnPoolLnParams cn_poolln_params(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, const float* gamma, const float* beta, float eps,
                                int B, int hw, int C) {
    CnPoolLnParams p = zeroed<CnPoolLnParams>();
    set_planes(p, x_hi, x_lo, y_hi, y_lo);
    p.gamma = gamma; p.beta = beta; p.B = B; p.hw = hw; p.C = C; p.eps = eps;
    return p;
}

TokParams tok_params(const void* x_hi, const void* x_lo, const float* cls, const float* pos, void* y_hi, void* y_lo, int B, int T, int D) {
    TokParams p = zeroed<TokParams>();
    set_planes(p, x_hi, x_lo, y_hi, y_lo);
    p.cls = cls; p.pos = pos; p.T = T; p.D = D;
    p.chunks = (long long)B * p.T * (p.D >> 3);
    return p;
}

AttnParams attn_params(const void* qkv_hi, const void* qkv_lo, void* o_hi, void* o_lo, int B, int T, int heads) {
    AttnParams p = zeroed<AttnParams>();
    p.qkv_hi = (const half_t*)qkv_hi; p.qkv_lo = (const half_t*)qkv_lo; p.o_hi = (half_t*)o_hi; p.o_lo = (half_t*)o_lo;
    p.T = T; p.heads = heads; p.D = heads * AT_HD;
    p.units = (long long)B * p.heads;
    return p;
}

SeGateParams se_gate_params(const void* x_hi, const void* x_lo, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                            int hw, int pitch, int q) {
    SeGateParams p = zeroed<SeGateParams>();
    p.x_hi = (const half_t*)x_hi; p.x_lo = (const half_t*)x_lo;
    p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.gate = gate;
    p.hw = hw; p.pitch = pitch; p.q = q;
    return p;
}

SeScaleParams se_scale_params(const void* x_hi, const void* x_lo, const float* gate, void* y_hi, void* y_lo, int B, int hw, int pitch) {
    SeScaleParams p = zeroed<SeScaleParams>();
    set_planes(p, x_hi, x_lo, y_hi, y_lo);
    p.gate = gate; p.pitch = pitch;
    p.per_image = (long long)hw * (pitch / 8);
    p.units = (long long)B * p.per_image;
    return p;
}

ShuffleParams shuffle_params(const void* a_hi, const void* a_lo, int a_pitch, const void* b_hi, const void* b_lo, int b_pitch, void* y_hi,
                             void* y_lo, int B, int side, int bf, int hp) {
    ShuffleParams p = zeroed<ShuffleParams>();
    p.a_hi = (const half_t*)a_hi; p.a_lo = (const half_t*)a_lo; p.b_hi = (const half_t*)b_hi; p.b_lo = (const half_t*)b_lo;
    p.y_hi = (half_t*)y_hi; p.y_lo = (half_t*)y_lo;
    p.npix = (long long)B * side * side;
    p.a_pitch = a_pitch; p.b_pitch = b_pitch; p.bf = bf; p.hp = hp;
    return p;
}

Pool3cParams pool3c_params(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, int B, int hin, int stride, int pad, int pitch) {
    Pool3cParams p = zeroed<Pool3cParams>();
    set_planes(p, x_hi, x_lo, y_hi, y_lo);
    const int W = stride == 1 ? Pool3c<1>::W : Pool3c<2>::W;
    p.hin = hin; p.ho = pool3c_out_side(hin, stride, pad); p.pitch = pitch; p.pad = pad;
    p.runs = (p.ho + W - 1) / W;
    p.units = (long long)B * p.ho * p.runs * (pitch / 8);
    return p;
}

// ---- launchers of those ops ---------------------------------------------------------------------------------------------------------

// one concat_bn_relu_kernel launch
int launch_catnorm(mpx_engine* h, const CatNormParams& p, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    const unsigned long long units = (unsigned long long)p.npix * (unsigned)((p.c_end - p.c_begin) / 8);
    // Guideline 13 of the HIP guide for HBM-bound kernels: about 8 workgroups per CU, striding over the rest
    const unsigned grid = (unsigned)std::min<unsigned long long>((units + 255) / 256, (unsigned long long)h->num_cus * 8);
    hipLaunchKernelGGL(concat_bn_relu_kernel, dim3(grid), dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// The three depthwise + BatchNorm forms (mpx_dw.h)
enum DwForm {
    DW_RELU6,   // MobileNetV2: 3x3 + ReLU6, one thread per output pixel (dwconv3x3_bn_relu6_kernel)
    DW_LINEAR,  // ShuffleNetV2: 3x3, no activation, the run form without SiLU code
    DW_SILU     // EfficientNet-B0: 3x3 / 5x5, the run form with SiLU on load (act_in) and in the epilogue (act_out)
};

template <int K, bool SILU>
void launch_dw_run(const DwParams& p, unsigned grid, hipStream_t st) {
    if (p.stride == 1)
        hipLaunchKernelGGL((dwconv_bn_act_kernel<K, 1, SILU>), dim3(grid), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL((dwconv_bn_act_kernel<K, 2, SILU>), dim3(grid), dim3(256), 0, st, p);
}

// one depthwise + BatchNorm launch
int launch_dwconv(mpx_engine* h, const DwParams& p, DwForm form, int ksize, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    if (form == DW_RELU6) {
        const unsigned long long units = (unsigned long long)p.npix * (unsigned)(p.pitch / 8);
        // as launch_catnorm: about 8 workgroups per CU, striding over the rest
        const unsigned grid = (unsigned)std::min<unsigned long long>((units + 255) / 256, (unsigned long long)h->num_cus * 8);
        hipLaunchKernelGGL(dwconv3x3_bn_relu6_kernel, dim3(grid), dim3(256), 0, st, p);
        MPX_HIP(h, hipGetLastError());
        return 0;
    }
    // the run form: a unit is a run of 4 (stride 1) or 2 (stride 2) output pixels.  Grid cap, blocks per CU, measured at batch 2340 next to
    // the one-pixel form, ms at 8 / 4 / 2: 28x28 x 64 stride 1 0.262 / 0.263 / 0.257, 14x14 x 128 0.139 / 0.144 / 0.142,
    // 7x7 x 256 0.058 / 0.063 / 0.065; 56x56 x 64 stride 2 0.495 / 0.484 / 0.460, 28x28 x 128 0.249 / 0.250 / 0.237: 8 at stride 1, 2 at stride 2
    const int W = p.stride == 1 ? DwRun<3, 1>::W : DwRun<3, 2>::W;        // (W does not depend on K)
    const unsigned long long units = (unsigned long long)p.rows * (unsigned)((p.ho + W - 1) / W) * (unsigned)(p.pitch / 8);
    const unsigned grid = (unsigned)std::min<unsigned long long>((units + 255) / 256, (unsigned long long)h->num_cus * (p.stride == 1 ? 8 : 2));
    if (form == DW_LINEAR) launch_dw_run<3, false>(p, grid, st);
    else if (ksize == 3) launch_dw_run<3, true>(p, grid, st);
    else launch_dw_run<5, true>(p, grid, st);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// Grid of a ConvNeXt LayerNorm kernel (mpx_cnext.h): `units` slots of work, R = cn_slots(C) per workgroup and iteration, about `per_cu`
// workgroups per CU striding over the rest; max_blocks > 0 caps it further (the public entries' test hook: results do not depend on it)
unsigned cn_grid(const mpx_engine* h, long long units, int C, int per_cu, int max_blocks) {
    const long long R = cn_slots(C);
    long long grid = std::min<long long>((units + R - 1) / R, (long long)h->num_cus * per_cu);
    if (max_blocks > 0) grid = std::min<long long>(grid, max_blocks);
    return (unsigned)std::max<long long>(grid, 1);
}

// one dwconv7x7_ln_kernel launch.  The kernel holds 4 x 8 accumulators and one input row of 10 x 8 values per thread (two workgroups per
// CU): 4 workgroups per CU cover a tail
int launch_cn_dwln(mpx_engine* h, const CnDwLnParams& p, int max_blocks, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    hipLaunchKernelGGL(dwconv7x7_ln_kernel, dim3(cn_grid(h, p.units, p.C, 4, max_blocks)), dim3(CN_NT), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// one layernorm_c_kernel launch (ConvNeXt's and a ViT's LayerNorms; in_stride > 1: a ViT's encoder.ln)
int launch_cn_ln(mpx_engine* h, const CnLnParams& p, int max_blocks, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    hipLaunchKernelGGL(layernorm_c_kernel, dim3(cn_grid(h, p.rows, p.C, 8, max_blocks)), dim3(CN_NT), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// one tokens_assemble_kernel launch (mpx_attn.h)
int launch_tokens(mpx_engine* h, const TokParams& p, int max_blocks, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    long long grid = std::min<long long>((p.chunks + AT_NT - 1) / AT_NT, (long long)h->num_cus * 8);
    if (max_blocks > 0) grid = std::min<long long>(grid, max_blocks);
    hipLaunchKernelGGL(tokens_assemble_kernel, dim3((unsigned)std::max<long long>(grid, 1)), dim3(AT_NT), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// one attention_f16x3_kernel launch (mpx_attn.h): a unit is one (image, head); one head's V^T in the LDS (59 KB at T = 197) leaves room for
// two workgroups per CU
int launch_attn(mpx_engine* h, const AttnParams& p, int max_blocks, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    long long grid = std::min<long long>(p.units, (long long)h->num_cus * 2);
    if (max_blocks > 0) grid = std::min<long long>(grid, max_blocks);
    hipLaunchKernelGGL(attention_f16x3_kernel, dim3((unsigned)std::max<long long>(grid, 1)), dim3(AT_NT), at_lds_bytes(p.T), st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// one global_avgpool_ln_kernel launch
int launch_cn_poolln(mpx_engine* h, const CnPoolLnParams& p, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    hipLaunchKernelGGL(global_avgpool_ln_kernel, dim3(cn_grid(h, p.B, p.C, 8, 0)), dim3(CN_NT), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// dynamic LDS of one se_gate_kernel launch: part[S][pitch] | pooled[pitch] | s1[q]
size_t se_gate_lds(int pitch, int q) { return ((size_t)se_gate_slices(pitch) * pitch + pitch + q) * sizeof(float); }

// one se_gate_kernel launch, one workgroup per image.  relu: fc1's activation is ReLU (a RegNetY block's gate), not SiLU (EfficientNet's)
int launch_se_gate(mpx_engine* h, const SeGateParams& p, int B, bool relu, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    if (relu)
        hipLaunchKernelGGL(se_gate_kernel<true>, dim3((unsigned)B), dim3(256), se_gate_lds(p.pitch, p.q), st, p);
    else
        hipLaunchKernelGGL(se_gate_kernel<false>, dim3((unsigned)B), dim3(256), se_gate_lds(p.pitch, p.q), st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// one se_scale_kernel launch; about 8 workgroups per CU, striding over the rest
int launch_se_scale(mpx_engine* h, const SeScaleParams& p, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    const unsigned grid = (unsigned)std::min<long long>((p.units + 255) / 256, (long long)h->num_cus * 8);
    hipLaunchKernelGGL(se_scale_kernel, dim3(grid), dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// one shuffle2_concat_kernel launch.  The load width follows the alignment of the sources (mpx_shuffle.h): 8-byte loads when bf % 8 == 0,
// 2-byte loads otherwise.
int launch_shuffle(mpx_engine* h, const ShuffleParams& p, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    const unsigned long long units = (unsigned long long)p.npix * (unsigned)(2 * p.hp / 8);
    // as launch_dwconv: about 8 workgroups per CU, striding over the rest
    const unsigned grid = (unsigned)std::min<unsigned long long>((units + 255) / 256, (unsigned long long)h->num_cus * 8);
    if (p.bf % 8 == 0)
        hipLaunchKernelGGL(shuffle2_concat_kernel<true>, dim3(grid), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(shuffle2_concat_kernel<false>, dim3(grid), dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// one maxpool3x3_clip_kernel launch
int launch_pool3c(mpx_engine* h, const Pool3cParams& p, int stride, ProfTag tag, hipStream_t st) {
    ProfScope ps(h, st, 2, -1, tag);
    // a thread keeps the 18 (stride 1) or 15 (stride 2) loads per plane of its run in flight, so two workgroups per CU already cover the
    // latency; the grid strides over the rest
    const unsigned grid = (unsigned)std::min<long long>((p.units + 255) / 256, (long long)h->num_cus * 2);
    if (stride == 1)
        hipLaunchKernelGGL(maxpool3x3_clip_kernel<1>, dim3(grid), dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(maxpool3x3_clip_kernel<2>, dim3(grid), dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// The nine plane-to-plane pools (mpx_maxpool3x3s2 .. mpx_global_avgpool_logits) differ in their kernel, their number of 8-channel units and
// their grid rule only.  This is the rest: the engine's device, the profile record, the grid of 256-thread workgroups over `units`, the
// launch and its error check.
enum GridRule {
    GRID_CAP_16K,   // min(ceil(units / 256), 256 * 64), striding over the rest
    GRID_PER_CU,    // min(ceil(units / 256), 8 workgroups per CU), striding over the rest
    GRID_ALL        // ceil(units / 256): one thread per unit
};

template <class Kernel, class... Args>
int launch_planes(mpx_engine* h, Kernel kernel, size_t units, GridRule rule, ProfTag tag, void* stream, Args... args) {
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    ProfScope ps(h, st, 2, -1, tag);
    size_t grid = (units + 255) / 256;
    if (rule == GRID_CAP_16K) grid = std::min<size_t>(grid, 256 * 64);
    if (rule == GRID_PER_CU) grid = std::min<size_t>(grid, (size_t)h->num_cus * 8);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, st, args...);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// mpx_pack_conv_weights with the input's channel layout: in_hp = 0 puts logical input channel ci in column ci of its tap; in_hp > 0 (the
// layer reads a whole two-half stage map, mpx_shuffle.h: 2 * in_bf logical channels at pitch 2 * in_hp = cin_pad) puts ci < in_bf at ci and
// ci >= in_bf at in_hp + ci - in_bf; the columns of the gaps stay zero.  even_stem: the layer is a stem with an EVEN kernel that reads the
// padded NHWC4 staging (ConvNeXt's 4x4 stride-4 patchify conv, K = 4 * 32) -- the row-run layout, which the descriptor alone cannot ask for:
// cin = 3, k = 4, K = 128 is also a generic layout (cin_pad = 8), and that meaning stays mpx_pack_conv_weights'.
int pack_conv_weights(const mpx_conv_desc* d, int in_bf, int in_hp, const float* w, const float* conv_bias, const float* gamma,
                      const float* beta, const float* mean, const float* var, float eps, uint16_t* w_hi, uint16_t* w_lo, float* scale,
                      float* shift, bool even_stem = false);

}  // namespace

// =============================================================================================
extern "C" {

int mpx_pack_conv_weights(const mpx_conv_desc* d, const float* w, const float* conv_bias, const float* gamma,
                          const float* beta, const float* mean, const float* var, float eps, uint16_t* w_hi,
                          uint16_t* w_lo, float* scale, float* shift) {
    return pack_conv_weights(d, 0, 0, w, conv_bias, gamma, beta, mean, var, eps, w_hi, w_lo, scale, shift);
}

}  // extern "C"

namespace {

int pack_conv_weights(const mpx_conv_desc* d, int in_bf, int in_hp, const float* w, const float* conv_bias, const float* gamma,
                      const float* beta, const float* mean, const float* var, float eps, uint16_t* w_hi, uint16_t* w_lo, float* scale,
                      float* shift, bool even_stem) {
    if (!d || !w || !w_hi || !w_lo || !scale || !shift) return MPX_E_ARG;
    const int cin = d->cin, cout = d->cout, k = d->ksize, K = d->k_packed;
    if (k <= 0 || cin <= 0 || cout <= 0 || cout > d->cout_pad || d->cout_pad % 16 != 0) return MPX_E_ARG;
    // row-run layout (the layers that read the padded NHWC4 staging: the 7x7 stem, K = 224, and the VGG 3x3 first layer, K = 96): one
    // 32-wide K step per kernel row, 8 pixels x 4 channels.  (The CIFAR ResNet's 3-channel conv1 reads [H][W][32] planes: K = 288.)  Odd
    // k in [3, 7] only: no descriptor the generic layout accepts (k = 1, 2, 4, 8 with K = k * 32) changes meaning.
    // AlexNet's 11x11 first layer is the two-run form: 16 pixels x 4 channels = two K steps per kernel row, K = 11 * 64 = 704 (a
    // descriptor the generic layout refuses: 704 is not 121 * cin_pad).
    // A ViT's patchify stems (even_stem again: 16x16 stride 16 and 32x32 stride 32) are one p-pixel run per kernel row: K = 16 * 64 / 32 * 128.
    const bool patch_stem = even_stem && cin == 3 && ((k == 16 && K == 16 * 64) || (k == 32 && K == 32 * 128));
    const int run = (cin == 3 && k == 11 && K == 11 * 64) ? 64 : (patch_stem ? 4 * k : 32);
    const bool stem = run >= 64 || (cin == 3 && K == k * 32 && (k & 1) && k >= 3 && k <= 7) || (even_stem && cin == 3 && K == k * 32 && k <= 8);
    if (cin == 3 && k == kStemK && !stem) return MPX_E_ARG;
    // K = k*k*cin_pad: the input planes may carry more channels per pixel than the layer reads (small nets pad to 32)
    const int cin_pad = stem ? 0 : K / (k * k);
    if (!stem && (K != k * k * cin_pad || cin_pad < cin || K % 32 != 0)) return MPX_E_ARG;
    if (in_hp && (stem || in_bf <= 0 || in_hp < in_bf || cin != 2 * in_bf || cin_pad != 2 * in_hp)) return MPX_E_ARG;
    std::memset(w_hi, 0, (size_t)d->cout_pad * K * 2);
    std::memset(w_lo, 0, (size_t)d->cout_pad * K * 2);
    for (int co = 0; co < d->cout_pad; ++co) {
        scale[co] = 0.f;
        shift[co] = 0.f;
    }
    for (int co = 0; co < cout; ++co) {
        const float* wc = w + (size_t)co * cin * k * k;
        float mx = 0.f;
        for (int j = 0; j < cin * k * k; ++j) mx = std::fmax(mx, std::fabs(wc[j]));
        int e = 0;
        if (mx > 0.f && std::isfinite(mx)) {
            int ex;
            std::frexp(mx, &ex);          // mx = f * 2^ex, f in [0.5,1)  ->  mx*2^(10-ex) in [512,1024)
            e = 10 - ex;
        }
        auto put = [&](int kk, float v) {
            const float sv = std::ldexp(v, e);
            const half_t hi = (half_t)sv;
            const half_t lo = (half_t)(sv - (float)hi);
            const size_t at = w_packed_index(co, kk, K);
            w_hi[at] = half_bits(hi);
            w_lo[at] = half_bits(lo);
        };
        if (stem) {
            for (int ky = 0; ky < k; ++ky)
                for (int px = 0; px < k; ++px)
                    for (int c = 0; c < 3; ++c) put(ky * run + px * 4 + c, wc[((size_t)c * k + ky) * k + px]);
        } else {
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx)
                    for (int ci = 0; ci < cin; ++ci)
                        put((ky * k + kx) * cin_pad + (in_hp && ci >= in_bf ? in_hp + ci - in_bf : ci), wc[((size_t)ci * k + ky) * k + kx]);
        }
        // y = bn(conv(x) + conv_bias) = s * acc + (beta + (conv_bias - mean) * s); without BatchNorm: y = acc + beta (+ conv_bias)
        double s = 1.0, t = 0.0;
        const double cb = conv_bias ? (double)conv_bias[co] : 0.0;
        if (gamma) {
            s = (double)gamma[co] / std::sqrt((double)var[co] + (double)eps);
            t = (double)beta[co] + (cb - (double)mean[co]) * s;
        } else {
            t = (beta ? (double)beta[co] : 0.0) + cb;
        }
        scale[co] = (float)std::ldexp(s, -e);
        shift[co] = (float)t;
    }
    return 0;
}

// The packed planes of a grouped 3x3 layer (mpx_gconv.h) from torchvision's [cout][cin / groups][3][3]: per channel block of CB = max(cg, 16)
// channels, rows = its output channels, k = (ky * 3 + kx) * CB + (the input channel's index within the block).  Output channel co of group g
// reads input channels [g * cg, (g + 1) * cg): inside its block these are columns (g * cg - block * CB) + ci; every other column of the row
// (the other groups of a cg = 4 / 8 block) and the K padding behind tap 8 stay exact zeros.  Row scaling, scale and shift are
// pack_conv_weights'.
int pack_gconv_weights(const mpx_conv_desc* d, int groups, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                       float eps, uint16_t* w_hi, uint16_t* w_lo, float* scale, float* shift) {
    const int C = d->cout, cg = C / groups, cb = gconv_cb(cg), K = gconv_kp(cb);
    if (d->cin != C || C % groups || d->ksize != 3 || d->k_packed != K || d->cout_pad != C || C % cb || !gamma || !beta || !mean || !var) return MPX_E_ARG;
    std::memset(w_hi, 0, (size_t)C * K * 2);
    std::memset(w_lo, 0, (size_t)C * K * 2);
    for (int co = 0; co < C; ++co) {
        const float* wc = w + (size_t)co * cg * 9;
        float mx = 0.f;
        for (int j = 0; j < cg * 9; ++j) mx = std::fmax(mx, std::fabs(wc[j]));
        int e = 0;
        if (mx > 0.f && std::isfinite(mx)) {
            int ex;
            std::frexp(mx, &ex);
            e = 10 - ex;
        }
        const int blk = co / cb, r = co - blk * cb, c0 = co / cg * cg - blk * cb;
        for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < cg; ++ci) {
                const float sv = std::ldexp(wc[(size_t)ci * 9 + t], e);
                const half_t hi = (half_t)sv;
                const half_t lo = (half_t)(sv - (float)hi);
                const size_t at = gconv_w_index(blk, r, t * cb + c0 + ci, cb);
                w_hi[at] = half_bits(hi);
                w_lo[at] = half_bits(lo);
            }
        const double s = (double)gamma[co] / std::sqrt((double)var[co] + (double)eps);
        scale[co] = (float)std::ldexp(s, -e);
        shift[co] = (float)((double)beta[co] - (double)mean[co] * s);
    }
    return 0;
}

// The packed planes of a grouped 3x3 layer in mpx_gconvw.h's form from torchvision's [w][cg][3][3]: per group ceil(cg / 16) row fragments of 16
// output channels, k = (ky * 3 + kx) * cg + ci over the group's own cg input channels.  The rows >= cg of a group's last fragment and the K
// padding behind tap 8 stay exact zeros.  Row scaling, scale and shift are pack_gconv_weights'; scale and shift are indexed by the channel.
int pack_gconvw_weights(const mpx_conv_desc* d, int groups, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                        float eps, uint16_t* w_hi, uint16_t* w_lo, float* scale, float* shift) {
    if (groups <= 0 || d->cout % groups) return MPX_E_ARG;
    const int C = d->cout, cg = C / groups, K = gconvw_kp(cg), rows = groups * gconvw_rf(cg) * 16;
    if (d->cin != C || cg % 8 || d->ksize != 3 || d->k_packed != K || d->cout_pad != rows || !gamma || !beta || !mean || !var) return MPX_E_ARG;
    std::memset(w_hi, 0, (size_t)rows * K * 2);
    std::memset(w_lo, 0, (size_t)rows * K * 2);
    for (int r = 0; r < rows; ++r) scale[r] = shift[r] = 0.f;
    for (int co = 0; co < C; ++co) {
        const float* wc = w + (size_t)co * cg * 9;
        float mx = 0.f;
        for (int j = 0; j < cg * 9; ++j) mx = std::fmax(mx, std::fabs(wc[j]));
        int e = 0;
        if (mx > 0.f && std::isfinite(mx)) {
            int ex;
            std::frexp(mx, &ex);
            e = 10 - ex;
        }
        const int g = co / cg, r = co - g * cg;
        for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < cg; ++ci) {
                const float sv = std::ldexp(wc[(size_t)ci * 9 + t], e);
                const half_t hi = (half_t)sv;
                const half_t lo = (half_t)(sv - (float)hi);
                const size_t at = gconvw_w_index(g, r, t * cg + ci, cg);
                w_hi[at] = half_bits(hi);
                w_lo[at] = half_bits(lo);
            }
        const double s = (double)gamma[co] / std::sqrt((double)var[co] + (double)eps);
        scale[co] = (float)std::ldexp(s, -e);
        shift[co] = (float)((double)beta[co] - (double)mean[co] * s);
    }
    return 0;
}

}  // namespace

extern "C" {

int mpx_create(int arch_id, int max_batch, int device, mpx_engine** out) {
    if (!out || max_batch <= 0) return MPX_E_ARG;
    *out = nullptr;
    mpx_engine* h = new (std::nothrow) mpx_engine();
    if (!h) return MPX_E_NOMEM;
    h->arch = arch_id; h->max_batch = max_batch; h->device = device;
    int rc = build_topology(h);
    if (rc) { delete h; return rc; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { delete h; return (int)e; }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) h->num_cus = cus;
    }

    // one arena: scratch | input planes | activation planes | pooled | logits | stem planes and weights | weights | SE gates.  layout()
    // below is its ONE description: it hands every buffer its `take(bytes)` in order, and runs twice -- over a null base to count the bytes,
    // over the allocation to assign the pointers -- so that no buffer's size is written down a second time.
    const size_t in_elems = h->small ? (size_t)h->img * h->img * kSmallCPad : (size_t)MPX_IMG_PAD * MPX_IMG_PAD * 4;
    const size_t in_plane = round_up((size_t)max_batch * in_elems * 2 + 256, 256);
    const size_t pool_plane = round_up((size_t)max_batch * round_up(h->feat, kSmallCPad) * 2, 256);
    const size_t scratch_bytes = 4096 * sizeof(float);
    // the stem by superposition (ImageNet ResNets): pooled stem planes, fp32 stem weights + BatchNorm vectors, one image's table (worst case:
    // 49 entries per conv output pixel), the bit planes of one staging call
    const bool stemtab = stem_pool_eligible(h);
    const bool stemw = stemtab && !h->densenet;     // a DenseNet engine runs the fused stem + pool launch but keeps no stem table
    const int tab_nmb = (max_batch + 31) / 32 + 1;
    // (the table itself -- 3 * tab_int + tab_lab + tab_vec + tab_bits, 160 MB -- is allocated by the first mpx_stem_table_build: an engine that
    // only ever stages through K0, stem = "conv", never pays for it)
    h->tab_sizes[0] = stemtab ? round_up((size_t)(ST_NPIX + 1) * 4, 256) : 0;
    h->tab_sizes[1] = stemtab ? round_up((size_t)ST_MAX_ENTRIES * 4, 256) : 0;
    h->tab_sizes[2] = stemtab ? round_up((size_t)ST_MAX_ENTRIES * ST_C * 4, 256) : 0;
    h->tab_sizes[3] = stemtab ? round_up((size_t)4096 * tab_nmb * 4, 256) : 0;
    auto layout = [&](char* base) -> size_t {
        size_t off = 0;
        auto take = [&](size_t n) { char* r = base ? base + off : nullptr; off += n; return r; };
        // `count` elements rounded up to 256 bytes, for one pointer or for a pair of equal buffers (hi / lo planes, scale / shift vectors)
        auto f32 = [&](float*& q, size_t count) { q = (float*)take(round_up(count * 4, 256)); };
        auto f16 = [&](half_t*& q, size_t count) { q = (half_t*)take(round_up(count * 2, 256)); };
        auto f32x2 = [&](float*& q0, float*& q1, size_t count) { f32(q0, count); f32(q1, count); };
        auto f16x2 = [&](half_t*& q0, half_t*& q1, size_t count) { f16(q0, count); f16(q1, count); };
        h->seg_scratch = (float*)take(scratch_bytes);
        h->in_hi = (half_t*)take(in_plane);
        h->in_lo = (half_t*)take(in_plane);
        for (int b = 0; b < h->n_act_bufs; ++b)         // one size for all buffers, except where the topology sizes each (ViT)
            f16x2(h->act_hi[b], h->act_lo[b], (size_t)max_batch * (h->act_elems_buf[b] ? h->act_elems_buf[b] : h->act_elems_per_image));
        h->pool_hi = (half_t*)take(pool_plane);
        h->pool_lo = (half_t*)take(pool_plane);
        f32(h->logits, (size_t)max_batch * h->logit_pitch);
        if (h->small) f32(h->k0_scratch, (size_t)2 + 4096 + max_batch);
        if (stemtab) f16x2(h->stem_hi, h->stem_lo, (size_t)max_batch * ST_POOLED * ST_POOLED * ST_C);
        if (stemw) {
            f32(h->stem_w32, (size_t)ST_TAPS * 3 * ST_C);
            f32x2(h->stem_s32, h->stem_t32, ST_C);
        }
        for (ConvLayer& L : h->convs) {
            f16x2(L.w_hi, L.w_lo, (size_t)L.d.cout_pad * L.d.k_packed);
            f32x2(L.scale, L.shift, (size_t)L.d.cout_pad);
            if (L.fuse_main) {
                f16x2(L.fw_hi, L.fw_lo, (size_t)L.d.cout_pad * (L.d.cin + h->convs[L.fuse_partner].d.cin));
                f32x2(L.fscale, L.fshift, (size_t)L.d.cout_pad);
            }
        }
        for (TailBlock& tb : h->tails) f16x2(tb.w3p_hi, tb.w3p_lo, (size_t)BT_OUT * (tb.ds >= 0 ? 2 : 1) * BT_MID);
        for (NormLayer& nl : h->norms) f32x2(nl.scale, nl.shift, (size_t)nl.d.channels);
        for (DwLayer& D : h->dws) {
            f32(D.w, (size_t)D.ksize * D.ksize * D.d.pitch);
            f32x2(D.scale, D.shift, (size_t)D.d.pitch);
            if (D.ln) f32(D.bias, (size_t)D.d.pitch);
        }
        for (LnLayer& N : h->lnorms) f32x2(N.gamma, N.beta, (size_t)N.d.channels);
        if (h->vit) {
            f32(h->cls_token, (size_t)h->vit_D);
            f32(h->pos_emb, (size_t)h->vit_T * h->vit_D);
        }
        for (SeLayer& E : h->ses) {
            f32x2(E.w1, E.w2, (size_t)E.d.q * E.d.pitch);
            f32(E.b1, (size_t)E.d.q);
            f32(E.b2, (size_t)E.d.pitch);
        }
        if (h->se_pitch_max) f32(h->se_gate, (size_t)max_batch * h->se_pitch_max);
        return off;
    };
    const size_t total = layout(nullptr);
    e = hipMalloc((void**)&h->arena, total);
    if (e != hipSuccess) { delete h; return (int)e; }
    h->arena_bytes = total;
    layout(h->arena);
    h->slot_src.assign((size_t)max_batch, 0);
    // the never-written borders (ImageNet) / padding channels (small nets) of the input staging must be zero, and so must
    // the pooled planes' padding channels
    e = hipMemset(h->arena, 0, scratch_bytes + 2 * in_plane);
    if (e == hipSuccess) e = hipMemset(h->pool_hi, 0, 2 * pool_plane);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (const KernelLds& k : kKernelLds)
        if (e == hipSuccess) e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes);
    if (e != hipSuccess) { (void)hipFree(h->arena); delete h; return (int)e; }
    *out = h;
    return 0;
}

int mpx_destroy(mpx_engine* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    for (ProfRec& r : h->prof_pool) {
        (void)hipEventDestroy(r.t0);
        (void)hipEventDestroy(r.t1);
    }
    if (h->arena) (void)hipFree(h->arena);
    if (h->tab_arena) (void)hipFree(h->tab_arena);
    delete h;
    return 0;
}

const char* mpx_last_error(const mpx_engine* h) { return h ? h->err.c_str() : "null engine"; }
int mpx_max_batch(const mpx_engine* h) { return h ? h->max_batch : MPX_E_ARG; }
int mpx_num_cus(const mpx_engine* h) { return h ? h->num_cus : MPX_E_ARG; }
int mpx_last_conv_kernels(const mpx_engine* h) { return h ? (int)h->last_kernels : MPX_E_ARG; }
size_t mpx_workspace_bytes(const mpx_engine* h) { return h ? h->arena_bytes + h->tab_arena_bytes : 0; }
int mpx_num_convs(const mpx_engine* h) { return h ? (int)h->convs.size() : MPX_E_ARG; }
int mpx_describe_plan(int arch_id, char* buf, size_t cap, size_t* len) { return describe_plan_of(arch_id, buf, cap, len); }

int mpx_conv_info(const mpx_engine* h, int i, mpx_conv_desc* out) {
    if (!h || !out || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    *out = h->convs[i].d;
    return 0;
}

int mpx_set_conv_weights(mpx_engine* h, int i, const float* w, const float* conv_bias, const float* gamma, const float* beta,
                         const float* mean, const float* var, float eps) {
    if (!h) return MPX_E_ARG;
    if (i < 0 || i >= (int)h->convs.size() || !w) return fail(h, MPX_E_ARG, "set_conv_weights: bad layer index or null weight");
    ConvLayer& L = h->convs[i];
    const bool has_bn = L.d.bn_name[0] != 0;
    if (has_bn && (!gamma || !beta || !mean || !var)) return fail(h, MPX_E_ARG, "set_conv_weights: BatchNorm tensors missing for %s", L.d.name);
    if (!has_bn) gamma = nullptr;
    if (L.has_bias && has_bn && !conv_bias) return fail(h, MPX_E_ARG, "set_conv_weights: %s is a conv with bias; conv_bias missing", L.d.name);
    const size_t n = (size_t)L.d.cout_pad * L.d.k_packed;
    std::vector<uint16_t> hi(n), lo(n);
    std::vector<float> sc(L.d.cout_pad), sh(L.d.cout_pad);
    int rc = L.gw      ? pack_gconvw_weights(&L.d, L.groups, w, gamma, beta, mean, var, eps, hi.data(), lo.data(), sc.data(), sh.data())
           : L.groups > 1 ? pack_gconv_weights(&L.d, L.groups, w, gamma, beta, mean, var, eps, hi.data(), lo.data(), sc.data(), sh.data())
                          : pack_conv_weights(&L.d, L.in_bf, L.in_hp, w, conv_bias, gamma, beta, mean, var, eps, hi.data(), lo.data(), sc.data(), sh.data(),
                                              L.is_stem && !(L.d.ksize & 1));
    if (rc) return fail(h, rc, "pack failed for %s", L.d.name);
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipMemcpy(L.w_hi, hi.data(), n * 2, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(L.w_lo, lo.data(), n * 2, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(L.scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(L.shift, sh.data(), sh.size() * 4, hipMemcpyHostToDevice));
    L.loaded = true;
    if (L.is_stem && h->stem_w32) {
        // the stem by superposition works from the fp32 tensors themselves: weights tap-major [(ky * 7 + kx) * 3 + ch][cout], the
        // BatchNorm as y = acc * s + t with s = gamma / sqrt(var + eps), t = beta - mean * s (rounded to fp32 once)
        std::vector<float> wt((size_t)ST_TAPS * 3 * ST_C), bs(ST_C), bt(ST_C);
        for (int co = 0; co < ST_C; ++co) {
            for (int ch = 0; ch < 3; ++ch)
                for (int t = 0; t < ST_TAPS; ++t) wt[((size_t)t * 3 + ch) * ST_C + co] = w[((size_t)co * 3 + ch) * ST_TAPS + t];
            const double sd = (double)gamma[co] / std::sqrt((double)var[co] + (double)eps);
            bs[co] = (float)sd;
            bt[co] = (float)((double)beta[co] - (double)mean[co] * sd);
        }
        MPX_HIP(h, hipMemcpy(h->stem_w32, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
        MPX_HIP(h, hipMemcpy(h->stem_s32, bs.data(), bs.size() * 4, hipMemcpyHostToDevice));
        MPX_HIP(h, hipMemcpy(h->stem_t32, bt.data(), bt.size() * 4, hipMemcpyHostToDevice));
        h->stem_w_loaded = true;
        h->tab_S = -1;                  // a table built from the old weights is stale
    }
    if (TailBlock* tb = tail_of_conv3(h, i)) {
        if (tb->ds < 0) {               // identity tail: the permuted copy of this layer's own planes (scale / shift are shared)
            rc = upload_tail_planes(h, *tb, hi, lo, L.d.k_packed);
            if (rc) return rc;
        } else {
            tb->ready = false;          // rebuilt by build_fused below once both layers of the pair are in
        }
    }
    if (L.fuse_partner >= 0) {
        const size_t nw = (size_t)L.d.cout * L.d.cin;       // both layers of a pair are 1x1
        L.hw.assign(w, w + nw);
        L.hgamma.assign(gamma, gamma + L.d.cout); L.hbeta.assign(beta, beta + L.d.cout);
        L.hmean.assign(mean, mean + L.d.cout); L.hvar.assign(var, var + L.d.cout);
        L.heps = eps;
        ConvLayer& P = h->convs[L.fuse_partner];
        const int main = L.fuse_main ? i : L.fuse_partner;
        h->convs[main].fused_loaded = false;
        if (!P.hw.empty()) return build_fused(h, main);
    }
    return 0;
}

int mpx_set_conv_tile(mpx_engine* h, int i, int tile) {
    if (!h) return MPX_E_ARG;
    if (i < 0 || i >= (int)h->convs.size()) return fail(h, MPX_E_ARG, "set_conv_tile: bad layer index");
    ConvLayer& L = h->convs[i];
    if (tile < 0) tile = L.tile_default >= 0 ? L.tile_default : default_tile(L.d);
    const TileRow* r = find_tile(tile);
    if (!r) {
        std::string ids;
        for (const TileRow& k : kTiles) ids += (ids.empty() ? "" : ", ") + std::to_string(k.id);
        return fail(h, MPX_E_ARG, "set_conv_tile: unknown tile %d (product ids: %s)", tile, ids.c_str());
    }
    if (L.gw && tile != kGconvwTile && !eligible(*r, L))
        return fail(h, MPX_E_ARG, "set_conv_tile: tile %d: a grouped layer of this network runs the any-width grouped 3x3 kernel (tile %d), and tile %d where its shape is one of that kernel's (%s is not)", tile, kGconvwTile, kGconvTile, L.d.name);
    if (L.groups > 1 && !L.gw && tile != kGconvTile)
        return fail(h, MPX_E_ARG, "set_conv_tile: tile %d: a grouped layer runs the grouped 3x3 kernel (tile %d) only (%s is one)", tile, kGconvTile, L.d.name);
    if (L.epi_act && r->eligible)
        return fail(h, MPX_E_ARG, "set_conv_tile: tile %d: %s applies GELU in its epilogue, which only the generic kernel (tiles 0, 1, 2, 4 and 7) has", tile, L.d.name);
    if (!eligible(*r, L)) return fail(h, MPX_E_ARG, "set_conv_tile: tile %d: %s (%s is not one)", tile, r->refusal, L.d.name);
    L.tile = tile;
    return 0;
}

int mpx_get_conv_tile(const mpx_engine* h, int i) {
    if (!h || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    return h->convs[i].tile;
}

int mpx_weights_complete(const mpx_engine* h) {
    if (!h) return MPX_E_ARG;
    for (const ConvLayer& L : h->convs)
        if (!L.loaded) return 0;
    for (const NormLayer& nl : h->norms)
        if (!nl.loaded) return 0;
    for (const DwLayer& D : h->dws)
        if (!D.loaded) return 0;
    for (const SeLayer& E : h->ses)
        if (!E.loaded) return 0;
    for (const LnLayer& N : h->lnorms)
        if (!N.loaded) return 0;
    if (h->vit && !h->tokens_loaded) return 0;
    return 1;
}

int mpx_num_lnorms(const mpx_engine* h) { return h ? (int)h->lnorms.size() : MPX_E_ARG; }

int mpx_lnorm_info(const mpx_engine* h, int k, mpx_lnorm_desc* out) {
    if (!h || !out || k < 0 || k >= (int)h->lnorms.size()) return MPX_E_ARG;
    *out = h->lnorms[k].d;
    return 0;
}

int mpx_load_lnorm(mpx_engine* h, int k, const float* weight, const float* bias, float eps) {
    if (!h) return MPX_E_ARG;
    if (k < 0 || k >= (int)h->lnorms.size()) return fail(h, MPX_E_ARG, "load_lnorm: bad LayerNorm index %d (this engine has %d)", k, (int)h->lnorms.size());
    LnLayer& N = h->lnorms[k];
    if (!weight || !bias) return fail(h, MPX_E_ARG, "load_lnorm: weight or bias missing for %s", N.d.name);
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(h, MPX_E_ARG, "load_lnorm: eps must be finite and >= 0");
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipMemcpy(N.gamma, weight, (size_t)N.d.channels * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(N.beta, bias, (size_t)N.d.channels * 4, hipMemcpyHostToDevice));
    N.eps = eps;
    N.loaded = true;
    return 0;
}

int mpx_lnorm_params(const mpx_engine* h, int k, const float** weight, const float** bias, float* eps) {
    if (!h || k < 0 || k >= (int)h->lnorms.size()) return MPX_E_ARG;
    if (weight) *weight = h->lnorms[k].gamma;
    if (bias) *bias = h->lnorms[k].beta;
    if (eps) *eps = h->lnorms[k].eps;
    return 0;
}

int mpx_num_norms(const mpx_engine* h) { return h ? (int)h->norms.size() : MPX_E_ARG; }

int mpx_norm_info(const mpx_engine* h, int k, mpx_norm_desc* out) {
    if (!h || !out || k < 0 || k >= (int)h->norms.size()) return MPX_E_ARG;
    *out = h->norms[k].d;
    return 0;
}

int mpx_load_norm(mpx_engine* h, int k, const float* gamma, const float* beta, const float* mean, const float* var, float eps) {
    if (!h) return MPX_E_ARG;
    if (k < 0 || k >= (int)h->norms.size()) return fail(h, MPX_E_ARG, "load_norm: bad norm index %d (this engine has %d)", k, (int)h->norms.size());
    NormLayer& nl = h->norms[k];
    if (!gamma || !beta || !mean || !var) return fail(h, MPX_E_ARG, "load_norm: BatchNorm tensors missing for %s", nl.d.name);
    const int n = nl.d.channels;
    std::vector<float> sc(n), sh(n);
    for (int c = 0; c < n; ++c) {
        const double s = (double)gamma[c] / std::sqrt((double)var[c] + (double)eps);
        sc[c] = (float)s;
        sh[c] = (float)((double)beta[c] - (double)mean[c] * s);
    }
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipMemcpy(nl.scale, sc.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(nl.shift, sh.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    nl.loaded = true;
    return 0;
}

int mpx_norm_params(const mpx_engine* h, int k, const float** scale, const float** shift) {
    if (!h || !scale || !shift || k < 0 || k >= (int)h->norms.size()) return MPX_E_ARG;
    *scale = h->norms[k].scale;
    *shift = h->norms[k].shift;
    return 0;
}

// ---- input staging: what the entries that read an image and the entries that fill input slots share ----
extern "C++" {
// The image source of a staging entry into p: exactly one of u8 / f32, mean / std required for u8 and 0 / 1 where absent.
template <class P>
static int image_source(mpx_engine* h, const char* what, P& p, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float mean[3],
                        const float std[3]) {
    if ((img_u8_hwc == nullptr) == (img_f32_chw == nullptr)) return fail(h, MPX_E_ARG, "%s: exactly one of img_u8_hwc / img_f32_chw must be given", what);
    if (img_u8_hwc && (!mean || !std)) return fail(h, MPX_E_ARG, "%s: mean/std required for u8 input", what);
    p.img_u8 = img_u8_hwc; p.img_f32 = img_f32_chw;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = mean ? mean[c] : 0.f;
        p.std[c] = std ? std[c] : 1.f;
    }
    return 0;
}

// The tail of an apply entry: M rows of p into the input slots [p.slot0, p.slot0 + M), one block per 256 pixels and STAGE_MT rows.
template <class P>
static int launch_stage(mpx_engine* h, void (*kernel)(P), int M, size_t lds, void* stream, P& p) {
    p.out_hi = h->in_hi; p.out_lo = h->in_lo;
    p.size = MPX_IMG; p.pad_size = MPX_IMG_PAD; p.border = 3;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    ProfScope ps(h, st, 1, -1);
    dim3 grid((MPX_IMG * MPX_IMG + 255) / 256, (M + STAGE_MT - 1) / STAGE_MT);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, p);
    MPX_HIP(h, hipGetLastError());
    std::fill(h->slot_src.begin() + p.slot0, h->slot_src.begin() + p.slot0 + M, (uint8_t)1);
    return 0;
}

// The weight source of a soft_* entry into p: RISE's cells, shifts and grid geometry, or the explicit weight maps.
template <class WS>
static void soft_source(SoftParams& p, const void* mask, const void* mask2, int s) {
    if (WS::kLds) {
        p.cells = (const uint8_t*)mask; p.shift = (const int32_t*)mask2;
        p.s = s;
        p.cell = (MPX_IMG + s - 1) / s;
        p.U2 = 2 * (s + 1) * p.cell;
        p.f_U2 = (float)p.U2;
        p.inv_U2 = 1.0f / p.f_U2;
    } else {
        p.weights = (const float*)mask;
    }
}
}  // extern "C++"

// K0: on/off rows over a label map, the soft apply kernel with the on/off weight source (mpx_softmask.h)
int mpx_mask_apply_normalize(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const int32_t* seg,
                             const uint8_t* onoff, int M, int S, const float mean[3], const float std[3], int slot0,
                             float* out_f32_nchw, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "mask_apply_normalize: this engine runs one of the small networks; use mpx_mask_apply_minmax");       // wording 1 of 3
    SoftParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, "mask_apply_normalize", p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!seg || !onoff || M <= 0 || S <= 0) return fail(h, MPX_E_ARG, "mask_apply_normalize: null input or empty M/S");    // M == 0 is refused here; the soft and rank entries return 0
    // a slot overflow is MPX_E_STATE here and MPX_E_ARG in the soft and rank entries; slot0 + M is not widened here
    if (slot0 < 0 || slot0 + M > h->max_batch) return fail(h, MPX_E_STATE, "mask_apply_normalize: slots [%d,%d) exceed max_batch %d", slot0, slot0 + M, h->max_batch);
    const size_t lds = OnoffWeights::lds_bytes(S);
    if (lds > 64 * 1024) return fail(h, MPX_E_ARG, "mask_apply_normalize: S=%d too large (max %d)", S, 64 * 1024 / STAGE_MT);
    p.seg = seg; p.onoff = onoff; p.out_f32 = out_f32_nchw;
    p.M = M; p.S = S; p.slot0 = slot0;
    return launch_stage(h, softmask_apply_kernel<OnoffWeights>, M, lds, stream, p);
}

// ---- real-valued masks (mpx_softmask.h): explicit weights or RISE's grids, applied like K0 and summed with the scores ----
extern "C++" {
template <class WS>
static int soft_apply(mpx_engine* h, const char* what, const uint8_t* img_u8_hwc, const float* img_f32_chw, const void* mask, const void* mask2,
                      int M, int s, const float mean[3], const float std[3], int slot0, float* out_f32_nchw, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "%s: this engine runs one of the small networks, whose mask convention is mpx_mask_apply_minmax's", what);      // wording 2 of 3
    if (WS::kLds && (s < SM_S_MIN || s > SM_S_MAX)) return fail(h, MPX_E_ARG, "%s: s=%d outside [%d, %d]", what, s, SM_S_MIN, SM_S_MAX);
    SoftParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, what, p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!mask || (WS::kLds && !mask2)) return fail(h, MPX_E_ARG, "%s: null mask pointer", what);
    if (M < 0 || slot0 < 0 || (long long)slot0 + M > h->max_batch)
        return fail(h, MPX_E_ARG, "%s: slots [%d,%lld) outside [0, max_batch=%d)", what, slot0, (long long)slot0 + M, h->max_batch);
    if (M == 0) return 0;
    soft_source<WS>(p, mask, mask2, s);
    p.out_f32 = out_f32_nchw;
    p.M = M; p.slot0 = slot0;
    return launch_stage(h, softmask_apply_kernel<WS>, M, WS::lds_bytes(s), stream, p);
}

template <class WS>
static int soft_saliency(mpx_engine* h, const char* what, const void* mask, const void* mask2, const float* weight, int M, int s, float* sal,
                         void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "%s: this engine runs one of the small networks (no 224 x 224 input)", what);       // wording 3 of 3
    if (WS::kLds && (s < SM_S_MIN || s > SM_S_MAX)) return fail(h, MPX_E_ARG, "%s: s=%d outside [%d, %d]", what, s, SM_S_MIN, SM_S_MAX);
    if (!mask || (WS::kLds && !mask2) || !weight || !sal) return fail(h, MPX_E_ARG, "%s: null pointer", what);
    if (M < 0) return fail(h, MPX_E_ARG, "%s: M=%d", what, M);
    if (M == 0) return 0;
    SoftParams p;
    std::memset(&p, 0, sizeof p);
    soft_source<WS>(p, mask, mask2, s);
    p.score = weight; p.sal = sal; p.M = M;
    p.size = MPX_IMG; p.pad_size = MPX_IMG_PAD; p.border = 3;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(softmask_saliency_kernel<WS>, dim3((MPX_IMG * MPX_IMG + SM_SAL_THREADS - 1) / SM_SAL_THREADS), dim3(SM_SAL_THREADS),
                       WS::lds_bytes(s), st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

}  // extern "C++"

int mpx_softmask_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* weights, int M, const float mean[3],
                       const float std[3], int slot0, float* out_f32_nchw, void* stream) {
    return soft_apply<ExplicitWeights>(h, "softmask_apply", img_u8_hwc, img_f32_chw, weights, nullptr, M, 0, mean, std, slot0, out_f32_nchw, stream);
}

int mpx_rise_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const uint8_t* cells, const int32_t* shift, int M, int s,
                   const float mean[3], const float std[3], int slot0, float* out_f32_nchw, void* stream) {
    return soft_apply<RiseWeights>(h, "rise_apply", img_u8_hwc, img_f32_chw, cells, shift, M, s, mean, std, slot0, out_f32_nchw, stream);
}

static_assert(SOBOL_GRID_MAX * SOBOL_GRID_MAX <= SUR_S_MAX, "mpx_segment_paint paints the d * d cells of the largest grid");
// the rows [row0, row0 + M) of a Sobol total-order design, their weights gathered from A and B in the kernel (DesignWeights); with a fill
// image the blend variant of the apply kernel
int mpx_sobol_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* A, const float* B, int N, int d, int row0,
                    int M, const float* fill_f32_chw, const float mean[3], const float std[3], int slot0, float* out_f32_nchw, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "sobol_apply: this engine runs one of the small networks, whose mask convention is mpx_mask_apply_minmax's");
    if (d < SOBOL_GRID_MIN || d > SOBOL_GRID_MAX) return fail(h, MPX_E_ARG, "sobol_apply: d=%d outside [%d, %d]", d, SOBOL_GRID_MIN, SOBOL_GRID_MAX);
    const long long rows = (long long)N * (d * d + 1);
    if (N < 2 || rows > INT_MAX) return fail(h, MPX_E_ARG, "sobol_apply: N=%d designs of %d cells: N >= 2 and N * (d * d + 1) rows within int", N, d * d);
    SoftParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, "sobol_apply", p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!A || !B) return fail(h, MPX_E_ARG, "sobol_apply: null design pointer");
    if (M < 0 || row0 < 0 || (long long)row0 + M > rows)
        return fail(h, MPX_E_ARG, "sobol_apply: rows [%d,%lld) outside the design's [0, %lld)", row0, (long long)row0 + M, rows);
    if (slot0 < 0 || (long long)slot0 + M > h->max_batch)
        return fail(h, MPX_E_ARG, "sobol_apply: slots [%d,%lld) outside [0, max_batch=%d)", slot0, (long long)slot0 + M, h->max_batch);
    if (M == 0) return 0;
    p.A = A; p.B = B; p.fill = fill_f32_chw;
    p.N = N; p.d = d; p.row0 = row0;
    p.out_f32 = out_f32_nchw;
    p.M = M; p.slot0 = slot0;
    if (fill_f32_chw) return launch_stage(h, softmask_apply_kernel<DesignWeights, true>, M, DesignWeights::lds_bytes(d), stream, p);
    return launch_stage(h, softmask_apply_kernel<DesignWeights>, M, DesignWeights::lds_bytes(d), stream, p);
}

// one sliding box per row, the weight 0 inside and 1 outside synthesised in the kernel (BoxWeights); with a fill image the blend variant
int mpx_box_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const int32_t* boxes, int M, const float* fill_f32_chw,
                  const float mean[3], const float std[3], int slot0, float* out_f32_nchw, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "box_apply: this engine runs one of the small networks, whose mask convention is mpx_mask_apply_minmax's");
    SoftParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, "box_apply", p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!boxes) return fail(h, MPX_E_ARG, "box_apply: null box pointer");
    if (M < 0 || slot0 < 0 || (long long)slot0 + M > h->max_batch)
        return fail(h, MPX_E_ARG, "box_apply: slots [%d,%lld) outside [0, max_batch=%d)", slot0, (long long)slot0 + M, h->max_batch);
    if (M == 0) return 0;
    p.boxes = boxes; p.fill = fill_f32_chw;
    p.out_f32 = out_f32_nchw;
    p.M = M; p.slot0 = slot0;
    if (fill_f32_chw) return launch_stage(h, softmask_apply_kernel<BoxWeights, true>, M, BoxWeights::lds_bytes(0), stream, p);
    return launch_stage(h, softmask_apply_kernel<BoxWeights>, M, BoxWeights::lds_bytes(0), stream, p);
}

// one activation map of g x g cells per row, upsampled to 224 x 224 and clamped to [0, 1] in the kernel (MapWeights)
int mpx_cam_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* cells, int M, int g, const float mean[3],
                  const float std[3], int slot0, float* out_f32_nchw, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "cam_apply: this engine runs one of the small networks, whose mask convention is mpx_mask_apply_minmax's");
    SoftParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, "cam_apply", p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!cells) return fail(h, MPX_E_ARG, "cam_apply: null cells pointer");
    if (g < CAM_G_MIN || g > CAM_G_MAX) return fail(h, MPX_E_ARG, "cam_apply: g=%d outside [%d, %d]", g, CAM_G_MIN, CAM_G_MAX);
    if (M < 0 || slot0 < 0 || (long long)slot0 + M > h->max_batch)
        return fail(h, MPX_E_ARG, "cam_apply: slots [%d,%lld) outside [0, max_batch=%d)", slot0, (long long)slot0 + M, h->max_batch);
    if (M == 0) return 0;
    p.maps = cells; p.g = g;
    p.out_f32 = out_f32_nchw;
    p.M = M; p.slot0 = slot0;
    return launch_stage(h, softmask_apply_kernel<MapWeights>, M, MapWeights::lds_bytes(g), stream, p);
}

int mpx_softmask_saliency(mpx_engine* h, const float* weights, const float* weight, int M, float* sal, void* stream) {
    return soft_saliency<ExplicitWeights>(h, "softmask_saliency", weights, nullptr, weight, M, 0, sal, stream);
}

int mpx_rise_saliency(mpx_engine* h, const uint8_t* cells, const int32_t* shift, const float* weight, int M, int s, float* sal, void* stream) {
    return soft_saliency<RiseWeights>(h, "rise_saliency", cells, shift, weight, M, s, sal, stream);
}

// ---- many classes from the same forwards (mpx_saliency_classes.h): K gathers per row of logits, the saliency sum with a tile of classes ----
int mpx_softmax_gather_classes(mpx_engine* h, const float* logits, const int32_t* classes, int K, float* scores, int score_pitch, int B,
                               void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "softmax_gather_classes: this engine runs one of the small networks (no 224 x 224 input)");
    if (!logits || !scores) return fail(h, MPX_E_ARG, "softmax_gather_classes: null pointer");
    if (B <= 0 || K <= 0) return fail(h, MPX_E_ARG, "softmax_gather_classes: B=%d K=%d", B, K);
    if (score_pitch < K) return fail(h, MPX_E_ARG, "softmax_gather_classes: score_pitch=%d < K=%d", score_pitch, K);
    if (!classes && K != h->ncls) return fail(h, MPX_E_ARG, "softmax_gather_classes: classes == NULL means all %d classes, K=%d", h->ncls, K);
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(softmax_gather_classes_kernel, dim3((B + 3) / 4), dim3(256), 0, st, logits, classes, K, scores, score_pitch, B, h->ncls,
                       h->logit_pitch);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

extern "C++" {
template <class WS>
static int soft_saliency_classes(mpx_engine* h, const char* what, const void* mask, const void* mask2, const float* scores, int score_pitch,
                                 int M, int K, int s, float* sal, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "%s: this engine runs one of the small networks (no 224 x 224 input)", what);
    if (WS::kLds && (s < SM_S_MIN || s > SM_S_MAX)) return fail(h, MPX_E_ARG, "%s: s=%d outside [%d, %d]", what, s, SM_S_MIN, SM_S_MAX);
    if (!mask || (WS::kLds && !mask2) || !scores || !sal) return fail(h, MPX_E_ARG, "%s: null pointer", what);
    if (M <= 0 || K <= 0) return fail(h, MPX_E_ARG, "%s: M=%d K=%d", what, M, K);
    if (score_pitch < K) return fail(h, MPX_E_ARG, "%s: score_pitch=%d < K=%d", what, score_pitch, K);
    SoftParams p;
    std::memset(&p, 0, sizeof p);
    soft_source<WS>(p, mask, mask2, s);
    p.score = scores; p.sal = sal; p.M = M;
    p.size = MPX_IMG; p.pad_size = MPX_IMG_PAD; p.border = 3;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    const dim3 grid((MPX_IMG * MPX_IMG + SC_THREADS - 1) / SC_THREADS, (K + SC_KT - 1) / SC_KT);
    hipLaunchKernelGGL(saliency_classes_kernel<WS>, grid, dim3(SC_THREADS), WS::lds_bytes(s), st, p, score_pitch, K);
    MPX_HIP(h, hipGetLastError());
    return 0;
}
}  // extern "C++"

int mpx_softmask_saliency_classes(mpx_engine* h, const float* weights, const float* scores, int score_pitch, int M, int K, float* sal,
                                  void* stream) {
    return soft_saliency_classes<ExplicitWeights>(h, "softmask_saliency_classes", weights, nullptr, scores, score_pitch, M, K, 0, sal, stream);
}

int mpx_rise_saliency_classes(mpx_engine* h, const uint8_t* cells, const int32_t* shift, const float* scores, int score_pitch, int M, int K,
                              int s, float* sal, void* stream) {
    return soft_saliency_classes<RiseWeights>(h, "rise_saliency_classes", cells, shift, scores, score_pitch, M, K, s, sal, stream);
}

// ---- occlusion sensitivity (mpx_occlusion.h): the mean score drop over the boxes that cover a pixel, summed and divided on the device ----
int mpx_box_saliency_classes(mpx_engine* h, const int32_t* boxes, const float* scores, int score_pitch, const float* base, int M, int K,
                             float* sum, int32_t* cnt, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "box_saliency_classes: this engine runs one of the small networks (no 224 x 224 input)");
    if (!boxes || !scores || !base || !sum || !cnt) return fail(h, MPX_E_ARG, "box_saliency_classes: null pointer");
    if (M < 0 || K <= 0 || K > 65535 * SC_KT) return fail(h, MPX_E_ARG, "box_saliency_classes: M=%d K=%d", M, K);
    if (score_pitch < K) return fail(h, MPX_E_ARG, "box_saliency_classes: score_pitch=%d < K=%d", score_pitch, K);
    if (M == 0) return 0;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    const dim3 grid((MPX_IMG * MPX_IMG + OCC_THREADS - 1) / OCC_THREADS, (K + SC_KT - 1) / SC_KT);
    hipLaunchKernelGGL(box_saliency_classes_kernel, grid, dim3(OCC_THREADS), 0, st, boxes, scores, score_pitch, base, M, K, sum, cnt, MPX_IMG);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_box_saliency_mean(mpx_engine* h, const float* sum, const int32_t* cnt, int K, float* out, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "box_saliency_mean: this engine runs one of the small networks (no 224 x 224 input)");
    if (!sum || !cnt || !out) return fail(h, MPX_E_ARG, "box_saliency_mean: null pointer");
    if (K <= 0) return fail(h, MPX_E_ARG, "box_saliency_mean: K=%d", K);
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    const dim3 grid((MPX_IMG * MPX_IMG + 255) / 256, std::min(K, 1024));
    hipLaunchKernelGGL(box_saliency_mean_kernel, grid, dim3(256), 0, st, sum, cnt, K, out, MPX_IMG * MPX_IMG);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// ---- Score-CAM (mpx_cam.h): the tap of the pool's input, the normalised cells of every channel, the score-weighted sum and its upsampling ----
int mpx_pool_input(mpx_engine* h, void** hi, void** lo, int* side, int* channels, int* pitch, int* load) {
    if (!h) return MPX_E_ARG;
    if (!hi || !lo || !side || !channels || !pitch || !load) return fail(h, MPX_E_ARG, "pool_input: null pointer");
    if (h->small) return fail(h, MPX_E_STATE, "pool_input: arch %d is one of the small networks, whose maps no 224 x 224 mask is made from", h->arch);
    // the list the last forward ran (the four lists of an engine put the pool's input into buffers of their own); before any, the plain one
    const std::vector<Op>& ops = h->fwd_ops ? *h->fwd_ops : h->ops;
    for (const Op& o : ops) {
        int ld = -1;
        switch (o.kind) {
            case OP_AVGPOOL: case OP_AVGPOOLLN: case OP_AVGLOGITS: ld = 0; break;
            case OP_AVGPOOL6: ld = 1; break;
            case OP_AVGPOOLSILU: ld = 2; break;
            default: break;
        }
        if (ld < 0) continue;
        int c = h->ncls;                // OP_AVGLOGITS: the pooled map holds the classes
        if (o.kind != OP_AVGLOGITS) {
            c = 0;
            for (const ConvLayer& L : h->convs)
                if (L.is_fc) c = L.d.cin;
        }
        if (o.in < 0 || c <= 0 || c > o.c) return fail(h, MPX_E_INTERNAL, "pool_input: the pool of arch %d reads buffer %d with %d channels at pitch %d", h->arch, o.in, c, o.c);
        *hi = h->act_hi[o.in];
        *lo = h->act_lo[o.in];
        *side = o.hin; *channels = c; *pitch = o.c; *load = ld;
        return 0;
    }
    const char* family = h->vit ? "ViT" : (h->arch >= MPX_ARCH_ALEXNET && h->arch < MPX_ARCH_ALEXNET + 100) ? "AlexNet"
                         : (h->arch > MPX_ARCH_VGG && h->arch < MPX_ARCH_VGG_BN + 100) ? "VGG" : "this network";
    return fail(h, MPX_E_STATE, "pool_input: arch %d (%s) has no global average pool in front of its logits; the VGGs, AlexNet, ViT and the small networks have none",
                h->arch, family);
}

int mpx_planes_to_chw(mpx_engine* h, const void* in_hi, const void* in_lo, int slot, int side, int channels, int pitch, int load, float* out_f32,
                      void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_f32) return fail(h, MPX_E_ARG, "planes_to_chw: null pointer");
    if (side <= 0 || side > MPX_IMG || channels < 0 || pitch <= 0 || channels > pitch || load < 0 || load > 2)
        return fail(h, MPX_E_ARG, "planes_to_chw: side=%d channels=%d pitch=%d load=%d (0 < side <= %d, 0 <= channels <= pitch, load 0 plain / 1 clamp6 / 2 silu)",
                    side, channels, pitch, load, MPX_IMG);
    if (slot < 0 || (long long)slot >= h->max_batch) return fail(h, MPX_E_ARG, "planes_to_chw: slot %d outside [0, max_batch=%d)", slot, h->max_batch);
    if (channels == 0) return 0;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    const int hw = side * side;
    const size_t off = (size_t)slot * hw * pitch;
    const half_t* a = (const half_t*)in_hi + off;
    const half_t* b = (const half_t*)in_lo + off;
    const dim3 grid((channels + CAM_T - 1) / CAM_T, (hw + CAM_T - 1) / CAM_T);
    if (load == 0) hipLaunchKernelGGL(planes_to_chw_kernel<POOL_PLAIN>, grid, dim3(256), 0, st, a, b, hw, channels, pitch, out_f32);
    else if (load == 1) hipLaunchKernelGGL(planes_to_chw_kernel<POOL_CLAMP6>, grid, dim3(256), 0, st, a, b, hw, channels, pitch, out_f32);
    else hipLaunchKernelGGL(planes_to_chw_kernel<POOL_SILU>, grid, dim3(256), 0, st, a, b, hw, channels, pitch, out_f32);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_cam_cells(mpx_engine* h, const float* act, int C, int g, float* cells, float* lo, float* hi, uint8_t* valid, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "cam_cells: this engine runs one of the small networks (no 224 x 224 input)");
    if (!act || !cells || !lo || !hi || !valid) return fail(h, MPX_E_ARG, "cam_cells: null pointer");
    if (g < CAM_G_MIN || g > CAM_G_MAX) return fail(h, MPX_E_ARG, "cam_cells: g=%d outside [%d, %d]", g, CAM_G_MIN, CAM_G_MAX);
    if (C < 0) return fail(h, MPX_E_ARG, "cam_cells: C=%d", C);
    if (C == 0) return 0;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(cam_cells_kernel, dim3(C), dim3(256), 0, st, act, g, cells, lo, hi, valid);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_cam_combine(mpx_engine* h, const float* act, const float* scores, int score_pitch, int R, int g, int K, float* low, float* sal,
                    void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "cam_combine: this engine runs one of the small networks (no 224 x 224 input)");
    if (!low || !sal || ((!act || !scores) && R != 0)) return fail(h, MPX_E_ARG, "cam_combine: null pointer");     // R == 0 reads neither act nor scores
    if (g < CAM_G_MIN || g > CAM_G_MAX) return fail(h, MPX_E_ARG, "cam_combine: g=%d outside [%d, %d]", g, CAM_G_MIN, CAM_G_MAX);
    if (R < 0 || K <= 0 || K > 0x7fffffff / (CAM_G_MAX * CAM_G_MAX)) return fail(h, MPX_E_ARG, "cam_combine: R=%d K=%d", R, K);
    if (score_pitch < K) return fail(h, MPX_E_ARG, "cam_combine: score_pitch=%d < K=%d", score_pitch, K);
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    const int gg = g * g;
    hipLaunchKernelGGL(cam_low_kernel, dim3((K * gg + 255) / 256), dim3(256), 0, st, act, scores, score_pitch, R, gg, K, low);
    MPX_HIP(h, hipGetLastError());
    const dim3 grid((MPX_IMG * MPX_IMG + 255) / 256, std::min(K, 1024));
    hipLaunchKernelGGL(cam_sal_kernel, grid, dim3(256), 0, st, (const float*)low, g, K, sal);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// ---- a linear surrogate over on/off superpixel rows (mpx_surrogate.h): the fp64 moment sums of LIME / KernelSHAP, the paint per superpixel ----
// Neither entry asks what network the engine runs: both serve every engine, the small networks included.  Booked with the head (kind 3) in
// a profile, ProfTag() as every stand-alone entry.
int mpx_surrogate_accumulate(mpx_engine* h, const uint8_t* onoff, const float* weight, const float* scores, int score_pitch, int M, int S,
                             int K, double* A, double* B, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!onoff || !weight || !scores || !A || !B) return fail(h, MPX_E_ARG, "surrogate_accumulate: null pointer");
    if (M < 0 || K < 1 || K > 65535 * SUR_KT) return fail(h, MPX_E_ARG, "surrogate_accumulate: M=%d K=%d", M, K);
    if (S < 1 || S > SUR_S_MAX) return fail(h, MPX_E_ARG, "surrogate_accumulate: S=%d outside [1, %d]", S, SUR_S_MAX);
    if (score_pitch < K) return fail(h, MPX_E_ARG, "surrogate_accumulate: score_pitch=%d < K=%d", score_pitch, K);
    if (M == 0) return 0;
    SurParams p;
    std::memset(&p, 0, sizeof p);
    p.onoff = onoff; p.weight = weight; p.scores = scores;
    p.score_pitch = score_pitch; p.M = M; p.S = S; p.K = K;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    ProfScope ps(h, st, 3, -1);
    const int rows = (S + 1 + SUR_THREADS - 1) / SUR_THREADS;
    p.out = A;
    hipLaunchKernelGGL(surrogate_accumulate_kernel<true>, dim3(rows, (S + 1 + SUR_KT - 1) / SUR_KT), dim3(SUR_THREADS), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    p.out = B;
    hipLaunchKernelGGL(surrogate_accumulate_kernel<false>, dim3(rows, (K + SUR_KT - 1) / SUR_KT), dim3(SUR_THREADS), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_segment_paint(mpx_engine* h, const int32_t* seg, const float* value, int value_pitch, int S, int K, float* out, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!seg || !value || !out) return fail(h, MPX_E_ARG, "segment_paint: null pointer");
    if (K < 1 || K > 65535) return fail(h, MPX_E_ARG, "segment_paint: K=%d", K);
    if (S < 1 || S > SUR_S_MAX) return fail(h, MPX_E_ARG, "segment_paint: S=%d outside [1, %d]", S, SUR_S_MAX);
    if (value_pitch < S) return fail(h, MPX_E_ARG, "segment_paint: value_pitch=%d < S=%d", value_pitch, S);
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    ProfScope ps(h, st, 3, -1);
    const int npix = h->img * h->img;
    hipLaunchKernelGGL(segment_paint_kernel, dim3((npix + 255) / 256, K), dim3(256), 0, st, seg, value, value_pitch, S, npix, out);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

// ---- a second pixel source (mpx_rankmask.h): rows that select between the image and a fill image on a per-pixel rank, and RISE's blur ----
int mpx_rank_apply(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const int32_t* rank, const int32_t* thresh, int M,
                   const float* fill_f32_chw, int keep_top, const float mean[3], const float std[3], int slot0, float* out_f32_nchw,
                   void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "rank_apply: this engine runs one of the small networks, whose mask convention is mpx_mask_apply_minmax's");
    RankParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, "rank_apply", p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!rank || !thresh) return fail(h, MPX_E_ARG, "rank_apply: null rank or thresh pointer");
    if (keep_top != 0 && keep_top != 1) return fail(h, MPX_E_ARG, "rank_apply: keep_top=%d is neither 0 nor 1", keep_top);
    if (M < 0 || slot0 < 0 || (long long)slot0 + M > h->max_batch)
        return fail(h, MPX_E_ARG, "rank_apply: slots [%d,%lld) outside [0, max_batch=%d)", slot0, (long long)slot0 + M, h->max_batch);
    if (M == 0) return 0;
    p.rank = rank; p.thresh = thresh; p.fill = fill_f32_chw; p.out_f32 = out_f32_nchw;
    p.M = M; p.slot0 = slot0; p.keep_top = keep_top;
    return launch_stage(h, rank_apply_kernel, M, 0, stream, p);
}

int mpx_blur_fill(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const float* taps, int klen, const float mean[3],
                  const float std[3], float* out_f32_chw, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->small) return fail(h, MPX_E_STATE, "blur_fill: this engine runs one of the small networks (no 224 x 224 input)");
    BlurParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, "blur_fill", p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!taps || !out_f32_chw) return fail(h, MPX_E_ARG, "blur_fill: null taps or out pointer");
    if (klen < 1 || klen > BF_KMAX || (klen & 1) == 0) return fail(h, MPX_E_ARG, "blur_fill: klen=%d is not an odd number in [1, %d]", klen, BF_KMAX);
    if (out_f32_chw == img_f32_chw) return fail(h, MPX_E_ARG, "blur_fill: out_f32_chw must not be the image (every block reads its neighbours' pixels)");
    p.out = out_f32_chw;
    for (int k = 0; k < klen; ++k) p.taps[k] = taps[k];
    p.klen = klen; p.size = MPX_IMG;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    dim3 grid((MPX_IMG + BF_TW - 1) / BF_TW, (MPX_IMG + BF_TH - 1) / BF_TH, 3);
    hipLaunchKernelGGL(blur_fill_kernel, grid, dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_stem_table_build(mpx_engine* h, const uint8_t* img_u8_hwc, const float* img_f32_chw, const int32_t* seg, int S,
                         const float mean[3], const float std[3], void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->densenet) return fail(h, MPX_E_STATE, "stem_table_build: a DenseNet engine keeps no stem table; it stages through mpx_mask_apply_normalize");
    if (!h->stem_w32) return fail(h, MPX_E_STATE, "stem_table_build: this architecture has no 7x7 stem with a max pool%s", !h->small ? " (VGG, AlexNet, MobileNetV2, SqueezeNet, GoogLeNet, ShuffleNetV2, EfficientNet-B0, ConvNeXt, ViT, RegNetX and RegNetY stage through mpx_mask_apply_normalize)" : "");
    StemTabParams p;
    std::memset(&p, 0, sizeof p);
    if (const int rc = image_source(h, "stem_table_build", p, img_u8_hwc, img_f32_chw, mean, std)) return rc;
    if (!seg || S <= 0 || S > 4096) return fail(h, MPX_E_ARG, "stem_table_build: null label map or S outside [1, 4096]");
    if (!h->stem_w_loaded) return fail(h, MPX_E_STATE, "stem_table_build: layer 0 (%s) has no weights", h->convs[0].d.name);
    MPX_SET_DEVICE(h);
    if (!h->tab_arena) {            // first table of this engine: its 160 MB are allocated now, once (the only allocation behind the boundary after mpx_create)
        const size_t total = 3 * h->tab_sizes[0] + h->tab_sizes[1] + h->tab_sizes[2] + h->tab_sizes[3];
        MPX_HIP(h, hipMalloc((void**)&h->tab_arena, total));
        h->tab_arena_bytes = total;
        char* cur = h->tab_arena;
        auto take = [&](size_t n) { char* r = cur; cur += n; return r; };
        h->tab_cnt = (int*)take(h->tab_sizes[0]);
        h->tab_off = (int*)take(h->tab_sizes[0]);
        h->tab_heavy = (int*)take(h->tab_sizes[0]);
        h->tab_lab = (int*)take(h->tab_sizes[1]);
        h->tab_vec = (float*)take(h->tab_sizes[2]);
        h->tab_bits = (unsigned*)take(h->tab_sizes[3]);
    }
    p.seg = seg; p.S = S;
    p.w = h->stem_w32; p.cnt = h->tab_cnt; p.off = h->tab_off; p.lab = h->tab_lab; p.vec = h->tab_vec;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    ProfScope ps(h, st, 1, -1);
    hipLaunchKernelGGL(stemtab_count_kernel, dim3(ST_NPIX / 4), dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(stemtab_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)h->tab_cnt, h->tab_off);
    MPX_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(stemtab_fill_kernel, dim3(ST_NPIX / 4), dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(stemtab_heavy_kernel, dim3(1), dim3(1024), 0, st, (const int*)h->tab_off, h->tab_heavy, h->tab_heavy + ST_POOLED * ST_POOLED);
    MPX_HIP(h, hipGetLastError());
    h->tab_S = S;
    return 0;
}

int mpx_stem_table_apply(mpx_engine* h, const uint8_t* onoff, int M, int S, int slot0, void* stream) {
    if (!h) return MPX_E_ARG;
    if (h->densenet) return fail(h, MPX_E_STATE, "stem_table_apply: a DenseNet engine keeps no stem table; it stages through mpx_mask_apply_normalize");
    if (!h->stem_w32) return fail(h, MPX_E_STATE, "stem_table_apply: this architecture has no 7x7 stem with a max pool");
    if (!onoff || M <= 0) return fail(h, MPX_E_ARG, "stem_table_apply: null mask rows or empty M");
    if (h->tab_S < 0) return fail(h, MPX_E_STATE, "stem_table_apply: no table in place (mpx_stem_table_build first; loading layer 0 again discards it)");
    if (S != h->tab_S) return fail(h, MPX_E_ARG, "stem_table_apply: S=%d, the table was built with S=%d", S, h->tab_S);
    if (slot0 < 0 || slot0 + M > h->max_batch) return fail(h, MPX_E_STATE, "stem_table_apply: slots [%d,%d) exceed max_batch %d", slot0, slot0 + M, h->max_batch);
    const int nmb = (M + 31) / 32;
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    {
        ProfScope ps(h, st, 1, -1);
        hipLaunchKernelGGL(onoff_bitplanes_kernel, dim3((S * nmb + 255) / 256), dim3(256), 0, st, onoff, M, S, nmb, h->tab_bits);
        MPX_HIP(h, hipGetLastError());
    }
    StemApplyParams p;
    std::memset(&p, 0, sizeof p);
    p.off = h->tab_off; p.lab = h->tab_lab; p.vec = h->tab_vec; p.bits = h->tab_bits; p.s = h->stem_s32; p.t = h->stem_t32;
    p.out_hi = h->stem_hi; p.out_lo = h->stem_lo; p.nmb = nmb; p.M = M; p.slot0 = slot0;
    p.heavy_list = h->tab_heavy; p.heavy_count = h->tab_heavy + ST_POOLED * ST_POOLED;
    {
        ProfScope ps(h, st, OP_CONV, 0);        // the stem's work: booked on layer 0 like the stem + pool launch it replaces
        // the pooled pixels with many superpixels under one window first (their workgroups share a pixel's masks), then every pixel
        hipLaunchKernelGGL(stem_apply_heavy_kernel, dim3(h->num_cus, nmb), dim3(256), 0, st, p);
        MPX_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(stem_apply_kernel, dim3(ST_POOLED * ST_POOLED / 4, nmb), dim3(256), 0, st, p);
        MPX_HIP(h, hipGetLastError());
    }
    std::fill(h->slot_src.begin() + slot0, h->slot_src.begin() + slot0 + M, (uint8_t)2);
    return 0;
}

int mpx_mask_apply_minmax(mpx_engine* h, const float* img_f32_chw, const int32_t* seg, const uint8_t* removed, int M, int S,
                          int slot0, float* out_f32_nchw, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!h->small) return fail(h, MPX_E_STATE, "mask_apply_minmax: only the small networks (MNIST net, CIFAR ResNet) use this mask convention");
    if (!img_f32_chw || !seg || !removed || M <= 0 || S <= 0 || S > 4096) return fail(h, MPX_E_ARG, "mask_apply_minmax: null input, empty M/S or S > 4096");
    if (slot0 < 0 || slot0 + M > h->max_batch) return fail(h, MPX_E_STATE, "mask_apply_minmax: slots [%d,%d) exceed max_batch %d", slot0, slot0 + M, h->max_batch);
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    ProfScope ps(h, st, 1, -1);
    const int hw = h->img * h->img;
    float* stats = h->k0_scratch;
    float* mask_max = h->k0_scratch + 2 + 4096;
    hipLaunchKernelGGL(smallnet_image_stats_kernel, dim3(1), dim3(256), 0, st, img_f32_chw, seg, h->in_ch, hw, S, stats);
    MPX_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(smallnet_mask_max_kernel, dim3((M + 255) / 256), dim3(256), 0, st, removed, M, S, (const float*)stats, mask_max);
    MPX_HIP(h, hipGetLastError());
    SmallMaskParams p;
    std::memset(&p, 0, sizeof p);
    p.img = img_f32_chw; p.seg = seg; p.removed = removed; p.stats = stats; p.mask_max = mask_max;
    p.out_hi = h->in_hi; p.out_lo = h->in_lo; p.out_f32 = out_f32_nchw;
    p.C = h->in_ch; p.hw = hw; p.M = M; p.S = S; p.slot0 = slot0;
    hipLaunchKernelGGL(smallnet_mask_apply_kernel, dim3((hw + 255) / 256, M), dim3(256), 0, st, p);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_avgpool2_pad(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin,
                     int cin_p, int cout_p, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hin <= 0 || (hin & 1) || cin_p <= 0 || (cin_p & 7) || cout_p < cin_p || (cout_p & 7))
        return fail(h, MPX_E_ARG, "avgpool2_pad: bad arguments (hin even, channel counts multiples of 8, cout_p >= cin_p)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "avgpool2_pad: the planes must be 16-byte aligned");
    return launch_planes(h, avgpool2_pad_kernel, (size_t)B * (hin / 2) * (hin / 2) * (cout_p / 8), GRID_CAP_16K, ProfTag(), stream,
                         (const half_t*)in_hi, (const half_t*)in_lo, (half_t*)out_hi, (half_t*)out_lo, B, hin, cin_p, cout_p);
}

int mpx_geometry(const mpx_engine* h, int* image_size, int* in_channels, int* num_classes, int* logit_pitch) {
    if (!h) return MPX_E_ARG;
    if (image_size) *image_size = h->img;
    if (in_channels) *in_channels = h->in_ch;
    if (num_classes) *num_classes = h->ncls;
    if (logit_pitch) *logit_pitch = h->logit_pitch;
    return 0;
}

int mpx_conv_bn_act(mpx_engine* h, int i, const void* in_hi, const void* in_lo, const void* res_hi, const void* res_lo,
                    void* out_hi, void* out_lo, float* out_f32, int B, void* stream) {
    if (!h) return MPX_E_ARG;
    if (i < 0 || i >= (int)h->convs.size() || B <= 0) return fail(h, MPX_E_ARG, "conv_bn_act: bad layer index or batch");
    const ConvLayer& L = h->convs[i];
    if (L.is_stem) {
        if (in_hi || in_lo) return fail(h, MPX_E_ARG, "conv_bn_act: layer 0 reads the engine input staging; pass NULL inputs");
        if (B > h->max_batch) return fail(h, MPX_E_STATE, "conv_bn_act: B > max_batch");
    } else if (h->small && i == 0 && !in_hi && !in_lo) {
        in_hi = h->in_hi;               // the small networks' first conv reads the engine's [B][H][W][32] staging
        in_lo = h->in_lo;
        if (B > h->max_batch) return fail(h, MPX_E_STATE, "conv_bn_act: B > max_batch");
    } else if (!in_hi || !in_lo) {
        return fail(h, MPX_E_ARG, "conv_bn_act: null input planes");
    }
    if ((res_hi == nullptr) != (res_lo == nullptr)) return fail(h, MPX_E_ARG, "conv_bn_act: residual planes must come in pairs");
    if (L.is_fc ? (out_f32 == nullptr) : (out_f32 != nullptr || !out_hi || !out_lo))
        return fail(h, MPX_E_ARG, "conv_bn_act: fc writes out_f32, every other layer writes out_hi/out_lo");
    MPX_SET_DEVICE(h);
    return launch_conv(h, i, (const half_t*)in_hi, (const half_t*)in_lo, (const half_t*)res_hi, (const half_t*)res_lo,
                       (half_t*)out_hi, (half_t*)out_lo, out_f32, B, as_stream(stream));
}

int mpx_maxpool3x3s2(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin,
                     int c, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hin <= 0 || (hin & 1) || c <= 0 || (c & 7))
        return fail(h, MPX_E_ARG, "maxpool3x3s2: bad arguments (hin even, c multiple of 8)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "maxpool3x3s2: the planes must be 16-byte aligned");
    return launch_planes(h, maxpool3x3s2_kernel, (size_t)B * (hin / 2) * (hin / 2) * (c / 8), GRID_CAP_16K, ProfTag(), stream,
                         (const half_t*)in_hi, (const half_t*)in_lo, (half_t*)out_hi, (half_t*)out_lo, B, hin, c);
}

int mpx_maxpool2x2s2(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin,
                     int c, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hin <= 0 || (hin & 1) || c <= 0 || (c & 7))
        return fail(h, MPX_E_ARG, "maxpool2x2s2: bad arguments (hin even, c multiple of 8)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "maxpool2x2s2: the planes must be 16-byte aligned");
    return launch_planes(h, maxpool_s2p0_kernel<2>, (size_t)B * (hin / 2) * (hin / 2) * (c / 8), GRID_CAP_16K, ProfTag(), stream,
                         (const half_t*)in_hi, (const half_t*)in_lo, (half_t*)out_hi, (half_t*)out_lo, B, hin, c);
}

int mpx_maxpool3x3s2p0(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin,
                       int c, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hin < 3 || !(hin & 1) || c <= 0 || (c & 7))
        return fail(h, MPX_E_ARG, "maxpool3x3s2p0: bad arguments (hin odd and >= 3, c multiple of 8)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "maxpool3x3s2p0: the planes must be 16-byte aligned");
    const int ho = (hin - 3) / 2 + 1;
    return launch_planes(h, maxpool_s2p0_kernel<3>, (size_t)B * ho * ho * (c / 8), GRID_CAP_16K, ProfTag(), stream, (const half_t*)in_hi,
                         (const half_t*)in_lo, (half_t*)out_hi, (half_t*)out_lo, B, hin, c);
}

int mpx_maxpool3x3_clip(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin, int stride, int pad,
                        int pitch, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hin <= 0 || (stride != 1 && stride != 2) || (pad != 0 && pad != 1) || pitch <= 0 ||
        (pitch & 7) || pool3c_out_side(hin, stride, pad) <= 0)
        return fail(h, MPX_E_ARG, "maxpool3x3_clip: bad arguments (stride 1 or 2, pad 0 or 1, hin + 2 * pad >= 3, pitch a multiple of 8)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "maxpool3x3_clip: the planes must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_pool3c(h, pool3c_params(in_hi, in_lo, out_hi, out_lo, B, hin, stride, pad, pitch), stride, ProfTag(), as_stream(stream));
}

int mpx_num_clip_pools(const mpx_engine* h) { return h ? (int)h->pools3c.size() : MPX_E_ARG; }

int mpx_clip_pool_info(const mpx_engine* h, int k, int* hin, int* stride, int* pad, int* pitch) {
    if (!h || k < 0 || k >= (int)h->pools3c.size()) return MPX_E_ARG;
    const ClipPool& P = h->pools3c[k];
    if (hin) *hin = P.hin;
    if (stride) *stride = P.stride;
    if (pad) *pad = P.pad;
    if (pitch) *pitch = P.pitch;
    return 0;
}

int mpx_global_avgpool(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hw,
                       int c, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hw <= 0 || c <= 0 || (c & 7) || (long long)B * (c / 8) > 0x7fffffffLL)
        return fail(h, MPX_E_ARG, "global_avgpool: bad arguments (c multiple of 8)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "global_avgpool: the planes must be 16-byte aligned");
    return launch_planes(h, global_avgpool_kernel<POOL_PLAIN>, (size_t)B * (c / 8), GRID_ALL, ProfTag(), stream, (const half_t*)in_hi, (const half_t*)in_lo,
                         (half_t*)out_hi, (half_t*)out_lo, B, hw, c);
}

int mpx_concat_bn_relu(mpx_engine* h, const void* fresh_hi, const void* fresh_lo, int g, int fresh_stride, void* raw_hi, void* raw_lo,
                       int c_total, int c_old, const float* scale, const float* shift, void* out_hi, void* out_lo, int c_norm,
                       long long npix, void* stream) {
    if (!h) return MPX_E_ARG;
    const bool fresh = fresh_hi != nullptr, norm = out_hi != nullptr;
    if (!raw_hi || !raw_lo || (fresh_hi == nullptr) != (fresh_lo == nullptr) || (out_hi == nullptr) != (out_lo == nullptr) || (!fresh && !norm))
        return fail(h, MPX_E_ARG, "concat_bn_relu: raw planes and at least one of fresh / out planes, planes in pairs");
    if (npix <= 0 || c_total <= 0 || (c_total & 7) || c_old < 0 || (c_old & 7))
        return fail(h, MPX_E_ARG, "concat_bn_relu: npix > 0, c_total a positive multiple of 8, c_old a multiple of 8");
    if (fresh ? (g <= 0 || (g & 7) || fresh_stride < g || (fresh_stride & 7) || (long long)c_old + g > c_total) : (g != 0))
        return fail(h, MPX_E_ARG, "concat_bn_relu: g a positive multiple of 8 with c_old + g <= c_total and fresh_stride >= g a multiple of 8 (g = 0 without fresh planes)");
    if (norm ? (!scale || !shift || c_norm <= 0 || (c_norm & 7) || (fresh ? c_norm != c_old + g : c_norm > c_total)) : (c_norm != 0 || scale || shift))
        return fail(h, MPX_E_ARG, "concat_bn_relu: c_norm = c_old + g with fresh planes, a positive multiple of 8 <= c_total without; scale / shift with out planes only");
    if (planes_misaligned({fresh_hi, fresh_lo, raw_hi, raw_lo, out_hi, out_lo, scale, shift}))
        return fail(h, MPX_E_ARG, "concat_bn_relu: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_catnorm(h, catnorm_params(fresh_hi, fresh_lo, g, fresh_stride, raw_hi, raw_lo, c_total, c_old, scale, shift, out_hi, out_lo, c_norm, npix),
                          ProfTag(), as_stream(stream));
}

int mpx_num_dwconvs(const mpx_engine* h) { return h ? (int)h->dws.size() : MPX_E_ARG; }

int mpx_dwconv_info(const mpx_engine* h, int k, mpx_dwconv_desc* out) {
    if (!h || !out || k < 0 || k >= (int)h->dws.size()) return MPX_E_ARG;
    *out = h->dws[k].d;
    return 0;
}

int mpx_load_dwconv(mpx_engine* h, int k, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps) {
    if (!h) return MPX_E_ARG;
    if (k < 0 || k >= (int)h->dws.size()) return fail(h, MPX_E_ARG, "load_dwconv: bad depthwise index %d (this engine has %d)", k, (int)h->dws.size());
    DwLayer& D = h->dws[k];
    if (D.ln) return fail(h, MPX_E_ARG, "load_dwconv: %s has a conv bias and a LayerNorm behind it; use mpx_load_dwconv_ln", D.d.name);
    if (!w || !gamma || !beta || !mean || !var) return fail(h, MPX_E_ARG, "load_dwconv: weight or BatchNorm tensors missing for %s", D.d.name);
    const int n = D.d.channels, pitch = D.d.pitch, taps = D.ksize * D.ksize;     // w: [channels][1][ksize][ksize]
    std::vector<float> wt((size_t)taps * pitch, 0.f), sc(pitch, 0.f), sh(pitch, 0.f);     // zeros on the padded channels
    for (int c = 0; c < n; ++c) {
        const int q = D.in_hp && c >= D.in_bf ? D.in_hp + c - D.in_bf : c;      // a two-half stage map: the channel's physical position
        for (int t = 0; t < taps; ++t) wt[(size_t)t * pitch + q] = w[(size_t)c * taps + t];
        const double s = (double)gamma[c] / std::sqrt((double)var[c] + (double)eps);
        sc[q] = (float)s;
        sh[q] = (float)((double)beta[c] - (double)mean[c] * s);
    }
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipMemcpy(D.w, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(D.scale, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(D.shift, sh.data(), sh.size() * 4, hipMemcpyHostToDevice));
    D.loaded = true;
    return 0;
}

int mpx_dwconv_params(const mpx_engine* h, int k, const float** w, const float** scale, const float** shift) {
    if (!h || !w || !scale || !shift || k < 0 || k >= (int)h->dws.size()) return MPX_E_ARG;
    *w = h->dws[k].w;
    *scale = h->dws[k].scale;
    *shift = h->dws[k].shift;
    return 0;
}

int mpx_dwconv3x3_bn_relu6(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* scale, const float* shift,
                           void* out_hi, void* out_lo, int B, int hin, int pitch, int stride, int clamp_in, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !w || !scale || !shift || !out_hi || !out_lo)
        return fail(h, MPX_E_ARG, "dwconv3x3_bn_relu6: null pointer");
    if (B <= 0 || hin <= 0 || pitch <= 0 || (pitch & 7) || (stride != 1 && stride != 2))
        return fail(h, MPX_E_ARG, "dwconv3x3_bn_relu6: B > 0, hin > 0, pitch a positive multiple of 8, stride 1 or 2");
    if (planes_misaligned({in_hi, in_lo, w, scale, shift, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "dwconv3x3_bn_relu6: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_dwconv(h, dw_params(in_hi, in_lo, out_hi, out_lo, w, scale, shift, B, hin, pitch, stride, clamp_in, 0, 0), DW_RELU6, 3, ProfTag(),
                         as_stream(stream));
}

int mpx_dwconv3x3_bn(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* scale, const float* shift, void* out_hi,
                     void* out_lo, int B, int hin, int pitch, int stride, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !w || !scale || !shift || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "dwconv3x3_bn: null pointer");
    if (B <= 0 || hin <= 0 || pitch <= 0 || (pitch & 7) || (stride != 1 && stride != 2))
        return fail(h, MPX_E_ARG, "dwconv3x3_bn: B > 0, hin > 0, pitch a positive multiple of 8, stride 1 or 2");
    if (planes_misaligned({in_hi, in_lo, w, scale, shift, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "dwconv3x3_bn: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_dwconv(h, dw_params(in_hi, in_lo, out_hi, out_lo, w, scale, shift, B, hin, pitch, stride, 0, 0, 0), DW_LINEAR, 3, ProfTag(),
                         as_stream(stream));
}

int mpx_dwconv_layout(const mpx_engine* h, int k, int* linear, int* bf, int* hp) {
    if (!h || k < 0 || k >= (int)h->dws.size()) return MPX_E_ARG;
    if (linear) *linear = h->dws[k].linear ? 1 : 0;
    if (bf) *bf = h->dws[k].in_bf;
    if (hp) *hp = h->dws[k].in_hp;
    return 0;
}

int mpx_dwconv_shape(const mpx_engine* h, int k, int* ksize, int* act_in, int* act_out) {
    if (!h || k < 0 || k >= (int)h->dws.size()) return MPX_E_ARG;
    if (ksize) *ksize = h->dws[k].ksize;
    if (act_in) *act_in = h->dws[k].act_in;
    if (act_out) *act_out = h->dws[k].act_out;
    return 0;
}

int mpx_dwconv_ln(const mpx_engine* h, int k, int* ln, const float** bias, float* eps) {
    if (!h || k < 0 || k >= (int)h->dws.size()) return MPX_E_ARG;
    if (ln) *ln = h->dws[k].ln ? 1 : 0;
    if (bias) *bias = h->dws[k].bias;
    if (eps) *eps = h->dws[k].eps;
    return 0;
}

int mpx_load_dwconv_ln(mpx_engine* h, int k, const float* w, const float* conv_bias, const float* ln_weight, const float* ln_bias, float eps) {
    if (!h) return MPX_E_ARG;
    if (k < 0 || k >= (int)h->dws.size()) return fail(h, MPX_E_ARG, "load_dwconv_ln: bad depthwise index %d (this engine has %d)", k, (int)h->dws.size());
    DwLayer& D = h->dws[k];
    if (!D.ln) return fail(h, MPX_E_ARG, "load_dwconv_ln: %s has a BatchNorm behind it, not a LayerNorm; use mpx_load_dwconv", D.d.name);
    if (!w || !conv_bias || !ln_weight || !ln_bias) return fail(h, MPX_E_ARG, "load_dwconv_ln: weight, bias or LayerNorm tensors missing for %s", D.d.name);
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(h, MPX_E_ARG, "load_dwconv_ln: eps must be finite and >= 0");
    const int n = D.d.channels, taps = D.ksize * D.ksize;      // w: [channels][1][7][7] -> tap-major [49][channels]; channels == pitch
    std::vector<float> wt((size_t)taps * n);
    for (int c = 0; c < n; ++c)
        for (int t = 0; t < taps; ++t) wt[(size_t)t * n + c] = w[(size_t)c * taps + t];
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipMemcpy(D.w, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(D.bias, conv_bias, (size_t)n * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(D.scale, ln_weight, (size_t)n * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(D.shift, ln_bias, (size_t)n * 4, hipMemcpyHostToDevice));
    D.eps = eps;
    D.loaded = true;
    return 0;
}

int mpx_conv_epilogue_act(const mpx_engine* h, int i, int* act) {
    if (!h || !act || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    *act = h->convs[i].epi_act;
    return 0;
}

int mpx_dwconv7x7_ln(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* conv_bias, const float* ln_weight,
                     const float* ln_bias, float eps, void* out_hi, void* out_lo, int B, int hin, int C, int ksize, int stride, int max_blocks,
                     void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !w || !conv_bias || !ln_weight || !ln_bias || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "dwconv7x7_ln: null pointer");
    if (ksize != CN_DW_K || stride != 1)
        return fail(h, MPX_E_ARG, "dwconv7x7_ln: ksize %d stride %d: this entry runs the 7x7 stride-1 layers with a LayerNorm behind them (3x3 and 5x5 layers run mpx_dwconv_bn_act)", ksize, stride);
    if (B <= 0 || hin <= 0 || C <= 0 || (C & 7) || C > 8 * CN_NT || !(eps >= 0.f) || (long long)B * hin * hin > 0x7fffffffLL)
        return fail(h, MPX_E_ARG, "dwconv7x7_ln: B > 0, hin > 0, C a positive multiple of 8 up to %d, eps >= 0", 8 * CN_NT);
    if (planes_misaligned({in_hi, in_lo, w, conv_bias, ln_weight, ln_bias, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "dwconv7x7_ln: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_cn_dwln(h, cn_dwln_params(in_hi, in_lo, out_hi, out_lo, w, conv_bias, ln_weight, ln_bias, eps, B, hin, C), max_blocks, ProfTag(),
                          as_stream(stream));
}

int mpx_layernorm_c(mpx_engine* h, const void* in_hi, const void* in_lo, const float* ln_weight, const float* ln_bias, float eps, void* out_hi,
                    void* out_lo, long long rows, int C, int max_blocks, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !ln_weight || !ln_bias || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "layernorm_c: null pointer");
    if (rows <= 0 || C <= 0 || (C & 7) || C > 8 * CN_NT || !(eps >= 0.f))
        return fail(h, MPX_E_ARG, "layernorm_c: rows > 0, C a positive multiple of 8 up to %d, eps >= 0", 8 * CN_NT);
    if (planes_misaligned({in_hi, in_lo, ln_weight, ln_bias, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "layernorm_c: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_cn_ln(h, cn_ln_params(in_hi, in_lo, out_hi, out_lo, ln_weight, ln_bias, eps, rows, 1, C), max_blocks, ProfTag(), as_stream(stream));
}

int mpx_global_avgpool_ln(mpx_engine* h, const void* in_hi, const void* in_lo, const float* ln_weight, const float* ln_bias, float eps,
                          void* out_hi, void* out_lo, int B, int hw, int C, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !ln_weight || !ln_bias || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "global_avgpool_ln: null pointer");
    if (B <= 0 || hw <= 0 || C <= 0 || (C & 7) || C > 8 * CN_NT || !(eps >= 0.f))
        return fail(h, MPX_E_ARG, "global_avgpool_ln: B > 0, hw > 0, C a positive multiple of 8 up to %d, eps >= 0", 8 * CN_NT);
    if (planes_misaligned({in_hi, in_lo, ln_weight, ln_bias, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "global_avgpool_ln: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_cn_poolln(h, cn_poolln_params(in_hi, in_lo, out_hi, out_lo, ln_weight, ln_bias, eps, B, hw, C), ProfTag(), as_stream(stream));
}

int mpx_conv_rows(const mpx_engine* h, int i, int* rows_per_image) {
    if (!h || !rows_per_image || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    *rows_per_image = h->convs[i].rows;
    return 0;
}

int mpx_num_attn(const mpx_engine* h) { return h ? (int)h->attns.size() : MPX_E_ARG; }

int mpx_attn_info(const mpx_engine* h, int k, mpx_attn_desc* out) {
    if (!h || !out || k < 0 || k >= (int)h->attns.size()) return MPX_E_ARG;
    *out = h->attns[k].d;
    return 0;
}

int mpx_load_tokens(mpx_engine* h, const float* class_token, const float* pos_embedding) {
    if (!h) return MPX_E_ARG;
    if (!h->vit) return fail(h, MPX_E_STATE, "load_tokens: this architecture has no class token and no position embedding (a ViT engine has)");
    if (!class_token || !pos_embedding) return fail(h, MPX_E_ARG, "load_tokens: class_token or encoder.pos_embedding missing");
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipMemcpy(h->cls_token, class_token, (size_t)h->vit_D * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(h->pos_emb, pos_embedding, (size_t)h->vit_T * h->vit_D * 4, hipMemcpyHostToDevice));
    h->tokens_loaded = true;
    return 0;
}

int mpx_token_params(const mpx_engine* h, const float** class_token, const float** pos_embedding, int* tokens, int* width) {
    if (!h) return MPX_E_ARG;
    if (class_token) *class_token = h->cls_token;
    if (pos_embedding) *pos_embedding = h->pos_emb;
    if (tokens) *tokens = h->vit_T;
    if (width) *width = h->vit_D;
    return 0;
}

int mpx_attention(mpx_engine* h, const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, int B, int T, int heads, int max_blocks,
                  void* stream) {
    if (!h) return MPX_E_ARG;
    if (!qkv_hi || !qkv_lo || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "attention: null pointer");
    if (T < 1 || T > AT_MAX_T) return fail(h, MPX_E_ARG, "attention: T = %d: a sequence has 1 .. %d tokens (one head's V^T must fit the LDS)", T, AT_MAX_T);
    if (heads < 1 || heads > 64) return fail(h, MPX_E_ARG, "attention: heads = %d: the width is D = heads * 64 with 1 .. 64 heads (head_dim is 64)", heads);
    if (B <= 0 || (long long)B * T > 0x7fffffffLL) return fail(h, MPX_E_ARG, "attention: B > 0 and B * T below 2^31");
    if (planes_misaligned({qkv_hi, qkv_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "attention: every plane must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_attn(h, attn_params(qkv_hi, qkv_lo, out_hi, out_lo, B, T, heads), max_blocks, ProfTag(), as_stream(stream));
}

int mpx_tokens_assemble(mpx_engine* h, const void* patch_hi, const void* patch_lo, const float* class_token, const float* pos_embedding,
                        void* out_hi, void* out_lo, int B, int T, int D, int max_blocks, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!h->vit) return fail(h, MPX_E_STATE, "tokens_assemble: this architecture has no token sequence (a ViT engine has)");
    if (!patch_hi || !patch_lo || !class_token || !pos_embedding || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "tokens_assemble: null pointer");
    if (T < 1) return fail(h, MPX_E_ARG, "tokens_assemble: T = %d: a sequence has at least the class token", T);
    if (B <= 0 || D <= 0 || (D & 7) || (long long)B * T > 0x7fffffffLL) return fail(h, MPX_E_ARG, "tokens_assemble: B > 0, D a positive multiple of 8, B * T below 2^31");
    if (planes_misaligned({patch_hi, patch_lo, class_token, pos_embedding, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "tokens_assemble: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_tokens(h, tok_params(patch_hi, patch_lo, class_token, pos_embedding, out_hi, out_lo, B, T, D), max_blocks, ProfTag(), as_stream(stream));
}

int mpx_layernorm_rows(mpx_engine* h, const void* in_hi, const void* in_lo, const float* ln_weight, const float* ln_bias, float eps, void* out_hi,
                       void* out_lo, long long rows, long long in_stride, int C, int max_blocks, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !ln_weight || !ln_bias || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "layernorm_rows: null pointer");
    if (rows <= 0 || in_stride < 1 || C <= 0 || (C & 7) || C > 8 * CN_NT || !(eps >= 0.f))
        return fail(h, MPX_E_ARG, "layernorm_rows: rows > 0, in_stride >= 1, C a positive multiple of 8 up to %d, eps >= 0", 8 * CN_NT);
    if (planes_misaligned({in_hi, in_lo, ln_weight, ln_bias, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "layernorm_rows: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_cn_ln(h, cn_ln_params(in_hi, in_lo, out_hi, out_lo, ln_weight, ln_bias, eps, rows, in_stride, C), max_blocks, ProfTag(),
                        as_stream(stream));
}

int mpx_conv_consumer_act(const mpx_engine* h, int i, int* act) {
    if (!h || !act || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    *act = h->convs[i].consumer_act;
    return 0;
}

int mpx_dwconv_bn_act(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w, const float* scale, const float* shift, void* out_hi,
                      void* out_lo, int B, int hin, int pitch, int ksize, int stride, int act_in, int act_out, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !w || !scale || !shift || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "dwconv_bn_act: null pointer");
    if (B <= 0 || hin <= 0 || pitch <= 0 || (pitch & 7) || (ksize != 3 && ksize != 5) || (stride != 1 && stride != 2) || (act_in != 0 && act_in != 1) ||
        (act_out != 0 && act_out != 1))
        return fail(h, MPX_E_ARG, "dwconv_bn_act: B > 0, hin > 0, pitch a positive multiple of 8, ksize 3 or 5, stride 1 or 2, act codes 0 (none) or 1 (SiLU)");
    if (planes_misaligned({in_hi, in_lo, w, scale, shift, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "dwconv_bn_act: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_dwconv(h, dw_params(in_hi, in_lo, out_hi, out_lo, w, scale, shift, B, hin, pitch, stride, 0, act_in, act_out), DW_SILU, ksize,
                         ProfTag(), as_stream(stream));
}

// mpx_se_gate / mpx_se_gate_relu: one set of argument checks, the fc1 activation apart
static int se_gate_entry(mpx_engine* h, const char* who, bool relu, const void* in_hi, const void* in_lo, const float* w1, const float* b1, const float* w2,
                  const float* b2, float* gate, int B, int hw, int pitch, int q, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !w1 || !b1 || !w2 || !b2 || !gate) return fail(h, MPX_E_ARG, "%s: null pointer", who);
    if (B <= 0 || hw <= 0 || pitch <= 0 || (pitch & 7) || q <= 0) return fail(h, MPX_E_ARG, "%s: B > 0, hw > 0, pitch a positive multiple of 8, q > 0", who);
    if (planes_misaligned({in_hi, in_lo, w1, b1, w2, b2, gate})) return fail(h, MPX_E_ARG, "%s: every pointer must be 16-byte aligned", who);
    if (se_gate_lds(pitch, q) > 64 * 1024) return fail(h, MPX_E_ARG, "%s: pitch %d and q %d need more than 64 KB of LDS", who, pitch, q);
    MPX_SET_DEVICE(h);
    return launch_se_gate(h, se_gate_params(in_hi, in_lo, w1, b1, w2, b2, gate, hw, pitch, q), B, relu, ProfTag(), as_stream(stream));
}

int mpx_se_gate(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                int B, int hw, int pitch, int q, void* stream) {
    return se_gate_entry(h, "se_gate", false, in_hi, in_lo, w1, b1, w2, b2, gate, B, hw, pitch, q, stream);
}

int mpx_se_gate_relu(mpx_engine* h, const void* in_hi, const void* in_lo, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* gate, int B, int hw, int pitch, int q, void* stream) {
    return se_gate_entry(h, "se_gate_relu", true, in_hi, in_lo, w1, b1, w2, b2, gate, B, hw, pitch, q, stream);
}

int mpx_se_scale(mpx_engine* h, const void* in_hi, const void* in_lo, const float* gate, void* out_hi, void* out_lo, int B, int hw, int pitch,
                 void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !gate || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "se_scale: null pointer");
    if (B <= 0 || hw <= 0 || pitch <= 0 || (pitch & 7)) return fail(h, MPX_E_ARG, "se_scale: B > 0, hw > 0, pitch a positive multiple of 8");
    if (planes_misaligned({in_hi, in_lo, gate, out_hi, out_lo})) return fail(h, MPX_E_ARG, "se_scale: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_se_scale(h, se_scale_params(in_hi, in_lo, gate, out_hi, out_lo, B, hw, pitch), ProfTag(), as_stream(stream));
}

int mpx_pack_gconvw_weights(int width, int groups, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                            uint16_t* w_hi, uint16_t* w_lo, float* scale, float* shift) {
    if (width <= 0 || groups <= 0 || width % groups || !w || !w_hi || !w_lo || !scale || !shift) return MPX_E_ARG;
    const int cg = width / groups;
    if (cg != 16 && cg != 24 && cg != 48 && cg != 56 && cg != 120) return MPX_E_ARG;
    mpx_conv_desc d;
    std::memset(&d, 0, sizeof d);
    d.cin = d.cout = width; d.ksize = 3; d.pad = 1; d.stride = 1;
    d.k_packed = gconvw_kp(cg);
    d.cout_pad = groups * gconvw_rf(cg) * 16;
    return pack_gconvw_weights(&d, groups, w, gamma, beta, mean, var, eps, w_hi, w_lo, scale, shift);
}

int mpx_gconvw3x3_bn_act(mpx_engine* h, const void* in_hi, const void* in_lo, const void* w_hi, const void* w_lo, const float* scale, const float* shift,
                         void* out_hi, void* out_lo, int B, int hin, int width, int groups, int in_pitch, int out_pitch, int stride, int relu,
                         void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !w_hi || !w_lo || !scale || !shift || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "gconvw3x3: null pointer");
    if (planes_misaligned({in_hi, in_lo, w_hi, w_lo, scale, shift, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "gconvw3x3: every pointer must be 16-byte aligned");
    if (B <= 0 || hin <= 0 || width <= 0 || groups <= 0 || width % groups || (stride != 1 && stride != 2))
        return fail(h, MPX_E_ARG, "gconvw3x3: B > 0, hin > 0, width a positive multiple of groups > 0, stride 1 or 2");
    const int cg = width / groups;
    if (cg != 16 && cg != 24 && cg != 48 && cg != 56 && cg != 120)
        return fail(h, MPX_E_ARG, "gconvw3x3: %d channels per group; the kernel has 16, 24, 48, 56 and 120", cg);
    if (in_pitch < width || (in_pitch & 7) || out_pitch < width || (out_pitch & 7))
        return fail(h, MPX_E_ARG, "gconvw3x3: both pitches must be multiples of 8 and at least the width %d", width);
    const int hout = (hin - 1) / stride + 1;
    if ((long long)B * hin * hin > 0x7fffffffLL || (long long)B * hout * hout > 0x7fffffffLL) return fail(h, MPX_E_ARG, "gconvw3x3: batch too large for 32-bit pixel indices");
    ConvParams p;
    std::memset(&p, 0, sizeof p);
    p.x_hi = (const half_t*)in_hi; p.x_lo = (const half_t*)in_lo; p.w_hi = (const half_t*)w_hi; p.w_lo = (const half_t*)w_lo;
    p.scale = scale; p.shift = shift; p.y_hi = (half_t*)out_hi; p.y_lo = (half_t*)out_lo;
    p.hin = hin; p.win = hin; p.pix_stride = in_pitch; p.ho = hout; p.wo = hout;
    p.kh = 3; p.kw = 3; p.stride = stride; p.pad = 1;
    p.ktot = gconvw_kp(cg); p.cout = out_pitch; p.M = B * hout * hout; p.relu = relu ? 1 : 0;
    MPX_SET_DEVICE(h);
    h->last_kernels = 0;
    gconvw_launch(width, groups, p, as_stream(stream));
    return launched(h, kGconvwTile);
}

int mpx_num_se(const mpx_engine* h) { return h ? (int)h->ses.size() : MPX_E_ARG; }

int mpx_se_info(const mpx_engine* h, int k, mpx_se_desc* out) {
    if (!h || !out || k < 0 || k >= (int)h->ses.size()) return MPX_E_ARG;
    *out = h->ses[k].d;
    return 0;
}

int mpx_se_act(const mpx_engine* h, int k, int* act) {
    if (!h || !act || k < 0 || k >= (int)h->ses.size()) return MPX_E_ARG;
    *act = h->ses[k].relu ? 1 : 0;
    return 0;
}

int mpx_load_se(mpx_engine* h, int k, const float* w1, const float* b1, const float* w2, const float* b2) {
    if (!h) return MPX_E_ARG;
    if (k < 0 || k >= (int)h->ses.size()) return fail(h, MPX_E_ARG, "load_se: bad SE index %d (this engine has %d)", k, (int)h->ses.size());
    SeLayer& E = h->ses[k];
    if (!w1 || !b1 || !w2 || !b2) return fail(h, MPX_E_ARG, "load_se: fc1 / fc2 weight or bias missing for %s", E.d.name);
    const int n = E.d.channels, pitch = E.d.pitch, q = E.d.q;
    // fc1.weight [q][n] -> [q][pitch] with zero columns on the pads; fc2.weight [n][q] -> j-major [q][pitch]; fc2.bias -> [pitch] with -inf on
    // the pads, whose gates se_gate_kernel then writes as exact zeros
    std::vector<float> a((size_t)q * pitch, 0.f), b((size_t)q * pitch, 0.f), c(pitch, -INFINITY);
    for (int j = 0; j < q; ++j)
        for (int ch = 0; ch < n; ++ch) {
            a[(size_t)j * pitch + ch] = w1[(size_t)j * n + ch];
            b[(size_t)j * pitch + ch] = w2[(size_t)ch * q + j];
        }
    for (int ch = 0; ch < n; ++ch) c[ch] = b2[ch];
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipMemcpy(E.w1, a.data(), a.size() * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(E.w2, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(E.b1, b1, (size_t)q * 4, hipMemcpyHostToDevice));
    MPX_HIP(h, hipMemcpy(E.b2, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    E.loaded = true;
    return 0;
}

int mpx_se_params(const mpx_engine* h, int k, const float** w1, const float** b1, const float** w2, const float** b2) {
    if (!h || !w1 || !b1 || !w2 || !b2 || k < 0 || k >= (int)h->ses.size()) return MPX_E_ARG;
    *w1 = h->ses[k].w1;
    *b1 = h->ses[k].b1;
    *w2 = h->ses[k].w2;
    *b2 = h->ses[k].b2;
    return 0;
}

int mpx_global_avgpool_silu(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hw, int c, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hw <= 0 || c <= 0 || (c & 7) || (long long)B * (c / 8) > 0x7fffffffLL)
        return fail(h, MPX_E_ARG, "global_avgpool_silu: bad arguments (c multiple of 8)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "global_avgpool_silu: the planes must be 16-byte aligned");
    return launch_planes(h, global_avgpool_kernel<POOL_SILU>, (size_t)B * (c / 8), GRID_ALL, ProfTag(), stream, (const half_t*)in_hi,
                         (const half_t*)in_lo, (half_t*)out_hi, (half_t*)out_lo, B, hw, c);
}

int mpx_shuffle2_concat(mpx_engine* h, const void* a_hi, const void* a_lo, int a_pitch, const void* b_hi, const void* b_lo, int b_pitch,
                        void* out_hi, void* out_lo, int B, int hw, int bf, int hp, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!a_hi || !a_lo || !b_hi || !b_lo || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "shuffle2_concat: null pointer");
    if (B <= 0 || hw <= 0 || bf <= 0 || (bf & 1) || hp < bf || (hp & 31) || a_pitch < bf || (a_pitch & 7) || b_pitch < bf || (b_pitch & 7))
        return fail(h, MPX_E_ARG, "shuffle2_concat: B > 0, hw > 0, bf even and > 0, hp >= bf a multiple of 32, pitches >= bf and multiples of 8");
    if (planes_misaligned({a_hi, a_lo, b_hi, b_lo, out_hi, out_lo}))
        return fail(h, MPX_E_ARG, "shuffle2_concat: every pointer must be 16-byte aligned");
    MPX_SET_DEVICE(h);
    return launch_shuffle(h, shuffle_params(a_hi, a_lo, a_pitch, b_hi, b_lo, b_pitch, out_hi, out_lo, B, hw, bf, hp), ProfTag(), as_stream(stream));
}

int mpx_num_shuffles(const mpx_engine* h) { return h ? (int)h->shuffles.size() : MPX_E_ARG; }

int mpx_shuffle_info(const mpx_engine* h, int k, int* hw, int* bf, int* hp, int* a_pitch, int* b_pitch) {
    if (!h || k < 0 || k >= (int)h->shuffles.size()) return MPX_E_ARG;
    const ShuffleOp& S = h->shuffles[k];
    if (hw) *hw = S.side;
    if (bf) *bf = S.bf;
    if (hp) *hp = S.hp;
    if (a_pitch) *a_pitch = S.a_pitch;
    if (b_pitch) *b_pitch = S.b_pitch;
    return 0;
}

int mpx_conv_in_slice(const mpx_engine* h, int i, int* pitch, int* offset, int* bf, int* hp) {
    if (!h || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    const ConvLayer& L = h->convs[i];
    if (pitch) *pitch = L.is_stem ? 4 : (L.x_pitch ? L.x_pitch : L.cin_pad);
    if (offset) *offset = L.x_offset;
    if (bf) *bf = L.in_bf;
    if (hp) *hp = L.in_hp;
    return 0;
}

int mpx_global_avgpool_clamp6(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hw,
                              int c, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hw <= 0 || c <= 0 || (c & 7) || (long long)B * (c / 8) > 0x7fffffffLL)
        return fail(h, MPX_E_ARG, "global_avgpool_clamp6: bad arguments (c multiple of 8)");
    // (no alignment check, unlike its eight siblings: DESIGN.md 31 records the gap; closing it would reject calls that are accepted today)
    return launch_planes(h, global_avgpool_kernel<POOL_CLAMP6>, (size_t)B * (c / 8), GRID_ALL, ProfTag(), stream, (const half_t*)in_hi,
                         (const half_t*)in_lo, (half_t*)out_hi, (half_t*)out_lo, B, hw, c);
}

int mpx_global_avgpool_logits(mpx_engine* h, const void* in_hi, const void* in_lo, float* out_f32, int B, int hw, int c, int out_pitch,
                              void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_f32 || B <= 0 || hw <= 0 || c <= 0 || (c & 7) || out_pitch < c || (long long)B * (c / 8) > 0x7fffffffLL)
        return fail(h, MPX_E_ARG, "global_avgpool_logits: bad arguments (c a multiple of 8, out_pitch >= c)");
    if (planes_misaligned({in_hi, in_lo})) return fail(h, MPX_E_ARG, "global_avgpool_logits: the planes must be 16-byte aligned");
    return launch_planes(h, global_avgpool_logits_kernel, (size_t)B * (c / 8), GRID_ALL, ProfTag(), stream, (const half_t*)in_hi,
                         (const half_t*)in_lo, out_f32, B, hw, c, out_pitch);
}

int mpx_conv_groups(const mpx_engine* h, int i, int* groups) {
    if (!h || !groups || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    *groups = h->convs[i].groups;
    return 0;
}

int mpx_conv_out_slice(const mpx_engine* h, int i, int* pitch, int* offset) {
    if (!h || !pitch || !offset || i < 0 || i >= (int)h->convs.size()) return MPX_E_ARG;
    const ConvLayer& L = h->convs[i];
    *pitch = L.y_pitch ? L.y_pitch : L.cout_store;
    *offset = L.y_pitch ? L.y_offset : 0;
    return 0;
}

int mpx_avgpool2x2s2(mpx_engine* h, const void* in_hi, const void* in_lo, void* out_hi, void* out_lo, int B, int hin, int c,
                     void* stream) {
    if (!h) return MPX_E_ARG;
    if (!in_hi || !in_lo || !out_hi || !out_lo || B <= 0 || hin <= 0 || (hin & 1) || c <= 0 || (c & 7))
        return fail(h, MPX_E_ARG, "avgpool2x2s2: bad arguments (hin even and > 0, c a positive multiple of 8)");
    if (planes_misaligned({in_hi, in_lo, out_hi, out_lo})) return fail(h, MPX_E_ARG, "avgpool2x2s2: the planes must be 16-byte aligned");
    return launch_planes(h, avgpool2x2s2_kernel, (size_t)B * (hin / 2) * (hin / 2) * (c / 8), GRID_PER_CU, ProfTag{PF_AVGPOOL2, 0}, stream,
                         (const half_t*)in_hi, (const half_t*)in_lo, (half_t*)out_hi, (half_t*)out_lo, B, hin, c);
}

int mpx_head_softmax_gather(mpx_engine* h, const float* logits, const int32_t* label, float* score, int32_t* pred,
                            int B, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!logits || !label || !score || !pred || B <= 0) return fail(h, MPX_E_ARG, "head_softmax_gather: null pointer or empty batch");
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    ProfScope ps(h, st, 3, -1);
    hipLaunchKernelGGL(head_softmax_gather_kernel, dim3((B + 3) / 4), dim3(256), 0, st, logits, label, score, pred, B,
                       h->ncls, h->logit_pitch);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_forward(mpx_engine* h, const int32_t* label, float* score, int32_t* pred, float* logits_out, int B,
                void* stream) {
    if (!h) return MPX_E_ARG;
    if (!label || !score || !pred || B <= 0) return fail(h, MPX_E_ARG, "forward: null pointer or empty batch");
    if (B > h->max_batch) return fail(h, MPX_E_STATE, "forward: B=%d exceeds max_batch=%d", B, h->max_batch);
    if (mpx_weights_complete(h) != 1) return fail(h, MPX_E_STATE, "forward: weights not loaded for every layer");
    float* logits = logits_out ? logits_out : h->logits;
    MPX_HIP(h, hipSetDevice(h->device));
    struct InForward {
        mpx_engine* e;
        explicit InForward(mpx_engine* e_) : e(e_) { e->in_forward = true; }
        ~InForward() { e->in_forward = false; }
    } scope(h);
    // (BUF_INPUT stays NULL: layer 0 reads the engine's own staging, mpx_conv_bn_act)
    auto hi = [&](int b) -> half_t* { return b == BUF_POOL ? h->pool_hi : (b == BUF_STEM ? h->stem_hi : (b >= 0 ? h->act_hi[b] : nullptr)); };
    auto lo = [&](int b) -> half_t* { return b == BUF_POOL ? h->pool_lo : (b == BUF_STEM ? h->stem_lo : (b >= 0 ? h->act_lo[b] : nullptr)); };
    const hipStream_t st = as_stream(stream);
    int rc = 0;
    bool skip_pool = false;
    // how the B slots were staged: by K0 into the input staging (the stem conv + max pool run here) or by mpx_stem_table_apply, which has
    // written the pooled stem planes already (the stem and the pool are skipped).  A batch staged by both is an error, not a guess.
    bool stem_done = false;
    {
        int n_tab = 0, n_k0 = 0;
        for (int i = 0; i < B; ++i) {
            n_tab += h->slot_src[i] == 2;
            n_k0 += h->slot_src[i] == 1;
        }
        if (n_tab && n_tab != B)
            return fail(h, MPX_E_STATE, "forward: %d of the %d slots were staged by mpx_stem_table_apply and %d by mpx_mask_apply_normalize; one forward takes one kind", n_tab, B, n_k0);
        stem_done = n_tab == B;
    }
    // layer1's block tails as single launches (mpx_btail.h) whenever their planes are in and no tile override asks for the
    // layer-by-layer kernels of those layers
    bool use_bt = h->fuse_bt && h->fuse_ds && tails_ready(h);
    for (const TailBlock& tb : h->tails)
        for (int li : {tb.c1, tb.c2, tb.c3, tb.next1})
            use_bt = use_bt && h->convs[li].tile == default_tile(h->convs[li].d);
    // layer2's pointwise tails likewise (bit 2); a tile override on one of a pair's two layers sends THAT pair through its two layers
    const bool use_pt = h->fuse_pt && h->fuse_ds && !h->ptails.empty();
    const std::vector<Op>& ops = use_pt ? (use_bt ? h->ops_pt : h->ops_pt0) : (use_bt ? h->ops_bt : h->ops);
    h->fwd_ops = &ops;
    for (size_t oi = 0; oi < ops.size(); ++oi) {
        const Op& o = ops[oi];
        if (stem_done && ((o.kind == OP_CONV && o.conv == 0) || (o.kind == OP_MAXPOOL && o.out == BUF_STEM))) continue;
        switch (o.kind) {
            case OP_BTAIL:
                rc = launch_btail(h, o.conv, hi(o.in), lo(o.in), hi(o.res), lo(o.res), hi(o.out), lo(o.out), hi(o.z), lo(o.z), B, as_stream(stream));
                break;
            case OP_PTAIL:
                if (ptail_in_use(h, o.conv)) {
                    rc = launch_ptail(h, o.conv, hi(o.in), lo(o.in), hi(o.res), lo(o.res), hi(o.out), lo(o.out), hi(o.z), lo(o.z), B, as_stream(stream));
                    break;
                }
                rc = mpx_conv_bn_act(h, h->ptails[o.conv].c3, hi(o.in), lo(o.in), hi(o.res), lo(o.res), hi(o.out), lo(o.out), nullptr, B, stream);
                if (!rc) rc = mpx_conv_bn_act(h, h->ptails[o.conv].next1, hi(o.out), lo(o.out), nullptr, nullptr, hi(o.z), lo(o.z), nullptr, B, stream);
                break;
            case OP_CONV:
                if (h->fuse_pool && o.conv == 0 && oi + 1 < ops.size() && ops[oi + 1].kind == OP_MAXPOOL && stem_pool_eligible(h) &&
                    h->convs[0].tile == 1) {
                    const Op& pool = ops[oi + 1];        // the stem writes the pooled planes; the pool op is skipped
                    rc = launch_stem_pool(h, hi(pool.out), lo(pool.out), B, as_stream(stream));
                    skip_pool = true;
                    break;
                }
                if (h->fuse_ds && h->convs[o.conv].fuse_partner >= 0) {
                    const ConvLayer& CL = h->convs[o.conv];
                    const ConvLayer& MAIN = CL.fuse_main ? CL : h->convs[CL.fuse_partner];
                    const TileRow* r = find_tile(MAIN.tile);
                    if (MAIN.fused_loaded && r && r->dual >= 0) {
                        if (!CL.fuse_main) break;       // the downsample conv runs inside its main conv's launch
                        rc = launch_conv_fused(h, o.conv, hi(o.in), lo(o.in), hi(o.in2), lo(o.in2), hi(o.out), lo(o.out), B, as_stream(stream));
                        break;
                    }
                }
                if (h->convs[o.conv].is_fc)
                    rc = mpx_conv_bn_act(h, o.conv, hi(o.in), lo(o.in), nullptr, nullptr, nullptr, nullptr, logits, B, stream);
                else
                    rc = mpx_conv_bn_act(h, o.conv, hi(o.in), lo(o.in), hi(o.res), lo(o.res), hi(o.out), lo(o.out), nullptr, B, stream);
                break;
            case OP_MAXPOOL:
                if (skip_pool) { skip_pool = false; break; }
                rc = mpx_maxpool3x3s2(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin, o.c, stream);
                break;
            case OP_MAXPOOL2: rc = mpx_maxpool2x2s2(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin, o.c, stream); break;
            case OP_MAXPOOL3P0: rc = mpx_maxpool3x3s2p0(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin, o.c, stream); break;
            case OP_AVGPOOL: rc = mpx_global_avgpool(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin * o.hin, o.c, stream); break;
            case OP_HEAD: rc = mpx_head_softmax_gather(h, logits, label, score, pred, B, stream); break;
            case OP_AVGPAD: rc = mpx_avgpool2_pad(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin, o.c >> 16, o.c & 0xffff, stream); break;
            case OP_AVGPOOL2: rc = mpx_avgpool2x2s2(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin, o.c, stream); break;
            case OP_AVGPOOL6: rc = mpx_global_avgpool_clamp6(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin * o.hin, o.c, stream); break;
            case OP_AVGLOGITS: rc = mpx_global_avgpool_logits(h, hi(o.in), lo(o.in), logits, B, o.hin * o.hin, o.c, h->logit_pitch, stream); break;
            case OP_MAXPOOL3C: {
                const ClipPool& P = h->pools3c[o.conv];
                rc = launch_pool3c(h, pool3c_params(hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, P.hin, P.stride, P.pad, P.pitch), P.stride,
                                   {PF_POOL3C, o.conv}, st);
                break;
            }
            case OP_DWCONV: {
                const DwLayer& D = h->dws[o.conv];
                const ProfTag tag{PF_DW, o.conv};
                if (D.ln)
                    rc = launch_cn_dwln(h, cn_dwln_params(hi(o.in), lo(o.in), hi(o.out), lo(o.out), D.w, D.bias, D.scale, D.shift, D.eps, B, D.d.hin, D.d.channels),
                                        0, tag, st);
                else
                    rc = launch_dwconv(h, dw_params(hi(o.in), lo(o.in), hi(o.out), lo(o.out), D.w, D.scale, D.shift, B, D.d.hin, D.d.pitch, D.d.stride, D.d.clamp_in,
                                                    D.act_in, D.act_out),
                                       D.mb ? DW_SILU : D.linear ? DW_LINEAR : DW_RELU6, D.ksize, tag, st);
                break;
            }
            case OP_SEGATE: {
                const SeLayer& E = h->ses[o.conv];
                rc = launch_se_gate(h, se_gate_params(hi(o.in), lo(o.in), E.w1, E.b1, E.w2, E.b2, h->se_gate, E.d.hw * E.d.hw, E.d.pitch, E.d.q), B, E.relu,
                                    {PF_SE_GATE, o.conv}, st);
                break;
            }
            case OP_SESCALE: {
                const SeLayer& E = h->ses[o.conv];
                rc = launch_se_scale(h, se_scale_params(hi(o.in), lo(o.in), h->se_gate, hi(o.out), lo(o.out), B, E.d.hw * E.d.hw, E.d.pitch),
                                     {PF_SE_SCALE, o.conv}, st);
                break;
            }
            case OP_AVGPOOLSILU: rc = mpx_global_avgpool_silu(h, hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, o.hin * o.hin, o.c, stream); break;
            case OP_LNORM: {        // rows: the pixels of a square map (ConvNeXt) or the tokens (ViT: o.hin = T)
                const LnLayer& N = h->lnorms[o.conv];
                const long long rows = (long long)B * o.hin * (h->vit ? 1 : o.hin);
                rc = launch_cn_ln(h, cn_ln_params(hi(o.in), lo(o.in), hi(o.out), lo(o.out), N.gamma, N.beta, N.eps, rows, 1, o.c), 0, {PF_LNORM, o.conv}, st);
                break;
            }
            case OP_LNORMROWS: {    // ViT: encoder.ln on the class-token row of each image (o.hin = T rows apart)
                const LnLayer& N = h->lnorms[o.conv];
                rc = launch_cn_ln(h, cn_ln_params(hi(o.in), lo(o.in), hi(o.out), lo(o.out), N.gamma, N.beta, N.eps, B, o.hin, o.c), 0, {PF_LNORM, o.conv}, st);
                break;
            }
            case OP_TOKENS:
                rc = launch_tokens(h, tok_params(hi(o.in), lo(o.in), h->cls_token, h->pos_emb, hi(o.out), lo(o.out), B, o.hin, o.c), 0, {PF_TOKENS, 0}, st);
                break;
            case OP_ATTN: {
                const AttnLayer& A = h->attns[o.conv];
                // (head_dim is AT_HD, build_topology_vit: the builder's D = heads * AT_HD is o.c)
                if (A.d.heads * A.d.head_dim != o.c) { rc = fail(h, MPX_E_INTERNAL, "attention: heads * 64 != D on %s", A.d.name); break; }
                rc = launch_attn(h, attn_params(hi(o.in), lo(o.in), hi(o.out), lo(o.out), B, A.d.tokens, A.d.heads), 0, {PF_ATTN, o.conv}, st);
                break;
            }
            case OP_AVGPOOLLN: {
                const LnLayer& N = h->lnorms[o.conv];
                rc = launch_cn_poolln(h, cn_poolln_params(hi(o.in), lo(o.in), hi(o.out), lo(o.out), N.gamma, N.beta, N.eps, B, o.hin * o.hin, o.c),
                                      {PF_LNORM, o.conv}, st);
                break;
            }
            case OP_SHUFFLE: {
                const ShuffleOp& S = h->shuffles[o.conv];
                rc = launch_shuffle(h, shuffle_params(hi(o.in), lo(o.in), S.a_pitch, hi(o.res) + S.b_offset, lo(o.res) + S.b_offset, S.b_pitch, hi(o.out), lo(o.out),
                                                      B, S.side, S.bf, S.hp), {PF_SHUFFLE, o.conv}, st);
                break;
            }
            case OP_CATNORM: {
                // append the fresh g channels (o.in, dense) to the block's raw concatenation (o.res) and write relu(bn(.)) of its
                // first o.c channels into o.out, in one launch
                const NormLayer& nl = h->norms[o.conv];
                rc = launch_catnorm(h, catnorm_params(hi(o.in), lo(o.in), o.g, o.g, hi(o.res), lo(o.res), o.ctot, o.c - o.g, nl.scale, nl.shift, hi(o.out), lo(o.out),
                                                      o.c, (long long)B * o.hin * o.hin), {PF_NORM, o.conv}, st);
                break;
            }
        }
        if (rc) return rc;
    }
    return 0;
}

int mpx_stem_conv_maxpool(mpx_engine* h, void* out_hi, void* out_lo, int B, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!out_hi || !out_lo || B <= 0) return fail(h, MPX_E_ARG, "stem + max pool: null pointer or empty batch");
    if (B > h->max_batch) return fail(h, MPX_E_STATE, "stem + max pool: B=%d exceeds max_batch=%d", B, h->max_batch);
    MPX_SET_DEVICE(h);
    return launch_stem_pool(h, (half_t*)out_hi, (half_t*)out_lo, B, as_stream(stream));
}

int mpx_set_fusion(mpx_engine* h, int mask) {
    if (!h) return MPX_E_ARG;
    h->fuse_pool = (mask & 1) != 0;
    h->fuse_ds = (mask & 1) != 0;
    h->fuse_bt = (mask & 2) != 0;
    h->fuse_pt = (mask & 4) != 0;
    return 0;
}

int mpx_bottleneck_tail(mpx_engine* h, int i, const void* t1_hi, const void* t1_lo, const void* x_hi, const void* x_lo,
                        void* out_hi, void* out_lo, void* next_hi, void* next_lo, int B, void* stream) {
    if (!h) return MPX_E_ARG;
    if (B <= 0 || (t1_hi == nullptr) != (t1_lo == nullptr) || !x_hi || !x_lo || !out_hi || !out_lo || !next_hi || !next_lo)
        return fail(h, MPX_E_ARG, "bottleneck_tail: null planes or empty batch");
    int ti = -1;
    for (size_t k = 0; k < h->tails.size(); ++k)
        if (h->tails[k].c2 == i) ti = (int)k;
    if (ti < 0) return fail(h, MPX_E_ARG, "bottleneck_tail: layer %d is not the conv2 of a block whose tail runs as one launch", i);
    {
        // the four plane pairs must not overlap: workgroups read t1's halo and the identity while others write out / next
        const TailBlock& tb = h->tails[ti];
        const size_t px = (size_t)B * h->convs[tb.c2].d.hin * h->convs[tb.c2].d.hin * sizeof(half_t);
        const size_t c_x = tb.ds >= 0 ? BT_MID : BT_OUT, c_next = (size_t)h->convs[tb.next1].d.cout;
        struct Range { const char* lo; size_t n; const char* what; };
        const Range r[8] = {{(const char*)t1_hi, px * BT_MID, "t1_hi"}, {(const char*)t1_lo, px * BT_MID, "t1_lo"},
                            {(const char*)x_hi, px * c_x, "x_hi"}, {(const char*)x_lo, px * c_x, "x_lo"},
                            {(const char*)out_hi, px * BT_OUT, "out_hi"}, {(const char*)out_lo, px * BT_OUT, "out_lo"},
                            {(const char*)next_hi, px * c_next, "next_hi"}, {(const char*)next_lo, px * c_next, "next_lo"}};
        for (int a = 0; a < 8; ++a)
            for (int b = a + 1; b < 8; ++b)
                if (r[a].lo && r[b].lo && r[a].lo < r[b].lo + r[b].n && r[b].lo < r[a].lo + r[a].n)
                    return fail(h, MPX_E_ARG, "bottleneck_tail: planes %s and %s overlap (all plane pairs must be distinct buffers)", r[a].what, r[b].what);
    }
    MPX_SET_DEVICE(h);
    return launch_btail(h, ti, (const half_t*)t1_hi, (const half_t*)t1_lo, (const half_t*)x_hi, (const half_t*)x_lo, (half_t*)out_hi,
                        (half_t*)out_lo, (half_t*)next_hi, (half_t*)next_lo, B, as_stream(stream));
}

int mpx_num_bottleneck_tails(const mpx_engine* h) { return h ? (int)h->tails.size() : MPX_E_ARG; }

int mpx_bottleneck_tail_info(const mpx_engine* h, int k, int* conv2, int* conv3, int* downsample, int* next_conv1) {
    if (!h || k < 0 || k >= (int)h->tails.size()) return MPX_E_ARG;
    if (conv2) *conv2 = h->tails[k].c2;         // (the block's own conv1 is the layer in front of it)
    if (conv3) *conv3 = h->tails[k].c3;
    if (downsample) *downsample = h->tails[k].ds;
    if (next_conv1) *next_conv1 = h->tails[k].next1;
    return 0;
}

int mpx_pointwise_tail(mpx_engine* h, int i, const void* t2_hi, const void* t2_lo, const void* x_hi, const void* x_lo,
                       void* out_hi, void* out_lo, void* next_hi, void* next_lo, int B, void* stream) {
    if (!h) return MPX_E_ARG;
    if (B <= 0 || !t2_hi || !t2_lo || !x_hi || !x_lo || !out_hi || !out_lo || !next_hi || !next_lo)
        return fail(h, MPX_E_ARG, "pointwise_tail: null planes or empty batch");
    int ti = -1;
    for (size_t k = 0; k < h->ptails.size(); ++k)
        if (h->ptails[k].c3 == i) ti = (int)k;
    if (ti < 0) return fail(h, MPX_E_ARG, "pointwise_tail: layer %d is not the conv3 of a block whose pointwise tail runs as one launch", i);
    {
        // the four plane pairs must not overlap: a workgroup reads t2 and the identity of its tiles while others write out / next
        const PointTail& pt = h->ptails[ti];
        const size_t px = (size_t)B * h->convs[pt.c3].d.hin * h->convs[pt.c3].d.hin * sizeof(half_t);
        struct Range { const char* lo; size_t n; const char* what; };
        const Range r[8] = {{(const char*)t2_hi, px * BtPw128::MID, "t2_hi"}, {(const char*)t2_lo, px * BtPw128::MID, "t2_lo"},
                            {(const char*)x_hi, px * BtPw128::OUT, "x_hi"}, {(const char*)x_lo, px * BtPw128::OUT, "x_lo"},
                            {(const char*)out_hi, px * BtPw128::OUT, "out_hi"}, {(const char*)out_lo, px * BtPw128::OUT, "out_lo"},
                            {(const char*)next_hi, px * BtPw128::C1, "next_hi"}, {(const char*)next_lo, px * BtPw128::C1, "next_lo"}};
        for (int a = 0; a < 8; ++a)
            for (int b = a + 1; b < 8; ++b)
                if (r[a].lo < r[b].lo + r[b].n && r[b].lo < r[a].lo + r[a].n)
                    return fail(h, MPX_E_ARG, "pointwise_tail: planes %s and %s overlap (all plane pairs must be distinct buffers)", r[a].what, r[b].what);
    }
    MPX_SET_DEVICE(h);
    return launch_ptail(h, ti, (const half_t*)t2_hi, (const half_t*)t2_lo, (const half_t*)x_hi, (const half_t*)x_lo, (half_t*)out_hi,
                        (half_t*)out_lo, (half_t*)next_hi, (half_t*)next_lo, B, as_stream(stream));
}

int mpx_num_pointwise_tails(const mpx_engine* h) { return h ? (int)h->ptails.size() : MPX_E_ARG; }

int mpx_pointwise_tail_info(const mpx_engine* h, int k, int* conv3, int* next_conv1) {
    if (!h || k < 0 || k >= (int)h->ptails.size()) return MPX_E_ARG;
    if (conv3) *conv3 = h->ptails[k].c3;
    if (next_conv1) *next_conv1 = h->ptails[k].next1;
    return 0;
}

int mpx_conv_dual_bn_act(mpx_engine* h, int i, const void* in_hi, const void* in_lo, const void* x_hi, const void* x_lo,
                         void* out_hi, void* out_lo, int B, void* stream) {
    if (!h) return MPX_E_ARG;
    if (i < 0 || i >= (int)h->convs.size() || B <= 0) return fail(h, MPX_E_ARG, "conv_dual_bn_act: bad layer index or batch");
    if (!h->convs[i].fuse_main) return fail(h, MPX_E_ARG, "conv_dual_bn_act: layer %d (%s) is not the last conv of a block with a downsample branch", i, h->convs[i].d.name);
    if (!in_hi || !in_lo || !x_hi || !x_lo || !out_hi || !out_lo) return fail(h, MPX_E_ARG, "conv_dual_bn_act: null planes");
    MPX_SET_DEVICE(h);
    return launch_conv_fused(h, i, (const half_t*)in_hi, (const half_t*)in_lo, (const half_t*)x_hi, (const half_t*)x_lo,
                             (half_t*)out_hi, (half_t*)out_lo, B, as_stream(stream));
}

int mpx_heatmap_accumulate(mpx_engine* h, const int32_t* seg, const uint8_t* onoff, const int32_t* pred,
                           const int32_t* label, int M, int S, float* heat, void* stream) {
    if (!h) return MPX_E_ARG;
    if (!seg || !onoff || !pred || !label || !heat || M <= 0 || S <= 0 || S > 4096)
        return fail(h, MPX_E_ARG, "heatmap_accumulate: null pointer, empty M/S or S > 4096");
    MPX_SET_DEVICE(h);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(heatmap_segment_count_kernel, dim3((S + 255) / 256), dim3(256), 0, st, onoff, pred, label, M, S,
                       h->seg_scratch);
    MPX_HIP(h, hipGetLastError());
    const int npix = h->img * h->img;
    hipLaunchKernelGGL(heatmap_gather_kernel, dim3((npix + 255) / 256), dim3(256), 0, st, seg, h->seg_scratch, S, npix, heat);
    MPX_HIP(h, hipGetLastError());
    return 0;
}

int mpx_input_planes(const mpx_engine* h, void** hi, void** lo) {
    if (!h || !hi || !lo) return MPX_E_ARG;
    *hi = h->in_hi;             // a pure getter: how the slots were staged (slot_src) is not touched -- a diagnostic call between
    *lo = h->in_lo;             // mpx_stem_table_apply and mpx_forward must not turn the forward onto stale input planes
    return 0;
}

int mpx_mark_input_staged(mpx_engine* h, int slot0, int M) {
    if (!h) return MPX_E_ARG;
    if (slot0 < 0 || M <= 0 || (long long)slot0 + M > h->max_batch)
        return fail(h, MPX_E_ARG, "mark_input_staged: slots [%d, %d) outside [0, max_batch=%d)", slot0, slot0 + M, h->max_batch);
    if (h->in_forward) return fail(h, MPX_E_STATE, "mark_input_staged: called during mpx_forward");
    // a caller that has WRITTEN the input planes of these slots by hand (mpx_input_planes) says so: the next mpx_forward runs the stem
    // conv + max pool on them, as after mpx_mask_apply_normalize, even if an earlier batch of the same slots came from mpx_stem_table_apply
    std::fill(h->slot_src.begin() + slot0, h->slot_src.begin() + slot0 + M, (uint8_t)1);
    return 0;
}

int mpx_stem_planes(const mpx_engine* h, void** hi, void** lo) {
    if (!h || !hi || !lo) return MPX_E_ARG;
    *hi = h->stem_hi;               // NULL for the small networks
    *lo = h->stem_lo;
    return 0;
}

int mpx_profile_enable(mpx_engine* h, int on) {
    if (!h) return MPX_E_ARG;
    if (on && h->prof_pool.empty()) {
        MPX_SET_DEVICE(h);
        h->prof_pool.resize(kProfilePairs);
        for (ProfRec& r : h->prof_pool) {
            MPX_HIP(h, hipEventCreate(&r.t0));
            MPX_HIP(h, hipEventCreate(&r.t1));
        }
    }
    h->prof_on = on != 0;
    return 0;
}

// The optional outputs of a profile collection beside the totals per kind (null: not wanted), in the order of the public argument lists
struct ProfOut {
    double *per_conv_ms, *per_norm_ms, *avgpool2_ms, *per_dw_ms, *per_clip_pool_ms, *per_shuffle_ms, *per_se_gate_ms, *per_se_scale_ms, *per_lnorm_ms,
        *per_attn_ms, *tokens_ms;
};

// Every mpx_profile_collect* entry: a record adds to the totals of its kind, to its conv layer, and to entry `index` of its family's list
static int profile_collect(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], const ProfOut& o) {
    if (!h || !ms_by_kind || !launches_by_kind) return MPX_E_ARG;
    if (h->prof_used == 0) return 0;
    const struct { double* ms; size_t n; } lists[PF_COUNT] = {
        {nullptr, 0},                               // PF_NONE
        {o.per_norm_ms, h->norms.size()},           // PF_NORM
        {o.avgpool2_ms, 1},                         // PF_AVGPOOL2
        {o.per_dw_ms, h->dws.size()},               // PF_DW
        {o.per_clip_pool_ms, h->pools3c.size()},    // PF_POOL3C
        {o.per_shuffle_ms, h->shuffles.size()},     // PF_SHUFFLE
        {o.per_se_gate_ms, h->ses.size()},          // PF_SE_GATE
        {o.per_se_scale_ms, h->ses.size()},         // PF_SE_SCALE
        {o.per_lnorm_ms, h->lnorms.size()},         // PF_LNORM
        {o.per_attn_ms, h->attns.size()},           // PF_ATTN
        {o.tokens_ms, 1},                           // PF_TOKENS
    };
    MPX_SET_DEVICE(h);
    MPX_HIP(h, hipEventSynchronize(h->prof_pool[h->prof_used - 1].t1));
    for (int i = 0; i < h->prof_used; ++i) {
        const ProfRec& r = h->prof_pool[i];
        float ms = 0.f;
        MPX_HIP(h, hipEventElapsedTime(&ms, r.t0, r.t1));
        ms_by_kind[r.kind] += ms;
        launches_by_kind[r.kind] += 1;
        if (o.per_conv_ms && r.kind == OP_CONV && r.conv >= 0) o.per_conv_ms[r.conv] += ms;
        if (lists[r.tag.family].ms && (size_t)r.tag.index < lists[r.tag.family].n) lists[r.tag.family].ms[r.tag.index] += ms;
    }
    h->prof_used = 0;
    return 0;
}

int mpx_profile_collect(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms});
}

int mpx_profile_collect_ex(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                           double* per_norm_ms, double* avgpool2_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms, per_norm_ms, avgpool2_ms});
}

int mpx_profile_collect_dw(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                           double* per_norm_ms, double* avgpool2_ms, double* per_dw_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms, per_norm_ms, avgpool2_ms, per_dw_ms});
}

int mpx_profile_collect_pool(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                             double* per_norm_ms, double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms, per_norm_ms, avgpool2_ms, per_dw_ms, per_clip_pool_ms});
}

int mpx_profile_collect_shuffle(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms,
                                double* per_norm_ms, double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms, per_norm_ms, avgpool2_ms, per_dw_ms, per_clip_pool_ms, per_shuffle_ms});
}

int mpx_profile_collect_se(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms, double* per_norm_ms,
                           double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms, double* per_se_gate_ms,
                           double* per_se_scale_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms, per_norm_ms, avgpool2_ms, per_dw_ms, per_clip_pool_ms, per_shuffle_ms,
                                                                     per_se_gate_ms, per_se_scale_ms});
}

int mpx_profile_collect_ln(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms, double* per_norm_ms,
                           double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms, double* per_se_gate_ms,
                           double* per_se_scale_ms, double* per_lnorm_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms, per_norm_ms, avgpool2_ms, per_dw_ms, per_clip_pool_ms, per_shuffle_ms,
                                                                     per_se_gate_ms, per_se_scale_ms, per_lnorm_ms});
}

int mpx_profile_collect_attn(mpx_engine* h, double ms_by_kind[4], long long launches_by_kind[4], double* per_conv_ms, double* per_norm_ms,
                             double* avgpool2_ms, double* per_dw_ms, double* per_clip_pool_ms, double* per_shuffle_ms, double* per_se_gate_ms,
                             double* per_se_scale_ms, double* per_lnorm_ms, double* per_attn_ms, double* tokens_ms) {
    return profile_collect(h, ms_by_kind, launches_by_kind, ProfOut{per_conv_ms, per_norm_ms, avgpool2_ms, per_dw_ms, per_clip_pool_ms, per_shuffle_ms,
                                                                     per_se_gate_ms, per_se_scale_ms, per_lnorm_ms, per_attn_ms, tokens_ms});
}

#ifdef MPX_DIAG
// diagnostic build only (not declared in include/mpx.h): DEV u64[8 * workgroups of the next conv launches]
int mpx_debug_set_stamps(mpx_engine* h, void* dev_buf) {
    if (!h) return MPX_E_ARG;
    h->stamps = (unsigned long long*)dev_buf;
    return 0;
}
#endif

double mpx_flops_per_forward(const mpx_engine* h) {
    if (!h) return 0.0;
    double macs = 0.0;
    for (const ConvLayer& L : h->convs)
        macs += (L.rows > 0 ? (double)L.rows : (double)L.d.hout * L.d.hout) * L.d.cout * (L.d.cin / L.groups) * L.d.ksize * L.d.ksize;
    for (const AttnLayer& A : h->attns) macs += 2.0 * A.d.tokens * A.d.tokens * A.d.head_dim * A.d.heads;      // Q K^T and P V
    for (const DwLayer& D : h->dws) {
        const int ho = dw_out_side(D.d.hin, D.d.stride);
        macs += (double)ho * ho * D.d.channels * D.ksize * D.ksize;
    }
    for (const SeLayer& E : h->ses) macs += 2.0 * E.d.channels * E.d.q;
    return 2.0 * macs;
}

}  // extern "C"
