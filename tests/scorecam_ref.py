"""What the Score-CAM tests share (test infrastructure only): the literal loop of one upsampling axis, the PUBLISHED order of the method
in torch (upsample every map with F.interpolate, then min-max; upsample every map, then sum at 224 x 224) as the reference the numpy
restatements of masks.py are weighed against, and the seeded activation maps and cells of the GPU cases.

The published order (Wang et al., CVPR-W 2020; pytorch-grad-cam's ScoreCAM), for act [C, g, g] and scores [C, K]:
    up_c   = interpolate(act_c, (224, 224), bilinear, align_corners=False)
    mask_c = (up_c - min up_c) / (max up_c - min up_c)                      a flat map is skipped
    sal_k  = relu(sum_c scores[c][k] * up_c)
masks.cam_combine sums at g x g and upsamples once; the two agree before the ReLU up to rounding, because the upsampling is linear."""
import numpy as np
import torch
import torch.nn.functional as F

IMG = 224
GRIDS = (2, 7, 13, 16)      # the smallest map, every ImageNet network's, SqueezeNet's, the largest (the largest LDS tile of the apply kernel)


def axis_loop(g):
    """(i0, i1, f) of one axis by a literal loop over y in Python integers; f = float32(r) / float32(448)."""
    i0, i1, f = [], [], []
    for y in range(IMG):
        t = max((2 * y + 1) * g - IMG, 0)
        q = t // (2 * IMG)
        r = t - q * 2 * IMG
        i0.append(q)
        i1.append(min(q + 1, g - 1))
        f.append(np.float32(r) / np.float32(2 * IMG))
    return np.array(i0), np.array(i1), np.array(f, dtype=np.float32)


def upsample_loop(G, pixels):
    """up(G) at the listed (y, x) by scalar fp32 arithmetic in the written order: every product and sum rounded on its own."""
    g = G.shape[0]
    i0, i1, f = axis_loop(g)
    one = np.float32(1.0)
    out = []
    for y, x in pixels:
        fy, fx = f[y], f[x]
        top = np.float32(np.float32(np.float32(one - fx) * G[i0[y], i0[x]]) + np.float32(fx * G[i0[y], i1[x]]))
        bot = np.float32(np.float32(np.float32(one - fx) * G[i1[y], i0[x]]) + np.float32(fx * G[i1[y], i1[x]]))
        out.append(np.float32(np.float32(np.float32(one - fy) * top) + np.float32(fy * bot)))
    return np.array(out, dtype=np.float32)


def torch_upsample(G, dtype=torch.float32):
    """F.interpolate of [N, g, g] to [N, 224, 224] in `dtype`."""
    t = torch.from_numpy(np.ascontiguousarray(G)).to(dtype)[None]
    return F.interpolate(t, size=(IMG, IMG), mode="bilinear", align_corners=False)[0]


def published_weights(act):
    """f32[C,224,224]: the published masks of act f32[C,g,g] in fp32 torch -- upsample, then min-max over the upsampled map."""
    up = torch_upsample(act)
    lo = up.amin(dim=(1, 2), keepdim=True)
    hi = up.amax(dim=(1, 2), keepdim=True)
    return ((up - lo) / (hi - lo)).numpy()


def published_combine(act, scores, dtype):
    """[K,224,224] in `dtype`: relu(sum_c scores[c][k] * up_c), every map upsampled first, summed at 224 x 224 in channel order."""
    up = torch_upsample(act, dtype)
    s = torch.from_numpy(np.ascontiguousarray(scores)).to(dtype)
    acc = torch.zeros(s.shape[1], IMG, IMG, dtype=dtype)
    for c in range(up.shape[0]):
        acc = acc + s[c][:, None, None] * up[c][None]
    return torch.relu(acc).numpy()


def activations(c, g, seed=0):
    """f32[c,g,g] post-ReLU-like maps (about a third of the cells exactly 0) with the special channels the cells kernel must get right
    planted from the front, as far as c allows: 0 an interior peak (one non-zero cell away from the border, where g allows one: no pixel
    centre reaches it), 1 a constant, 2 all zeros, 3 negative values only, 4 mixed signs."""
    rng = np.random.default_rng(1000 * g + c + seed)
    a = np.maximum(rng.standard_normal((c, g, g)).astype(np.float32), np.float32(-0.4)) + np.float32(0.4)
    a[0] = 0.0
    a[0, g // 2, min(g // 2, g - 1)] = 3.5
    if c > 1:
        a[1] = 2.25
    if c > 2:
        a[2] = 0.0
    if c > 3:
        a[3] = -np.abs(rng.standard_normal((g, g)).astype(np.float32)) - np.float32(0.5)
    if c > 4:
        a[4] = rng.standard_normal((g, g)).astype(np.float32)
    return np.ascontiguousarray(a)


def cells(m, g, seed=0):
    """f32[m,g,g] rows for the apply kernel: uniform in [-0.03, 1.08) -- what mpx_cam_cells writes, both sides of the clamp -- with an exact
    0.0, an exact 1.0, a value below 0 and one above 1 planted in row 0, and the LAST row all ones (the unmasked staging)."""
    rng = np.random.default_rng(77 * g + m + seed)
    c = (rng.random((m, g, g), dtype=np.float32) * np.float32(1.11) - np.float32(0.03)).astype(np.float32)
    c[0, 0, 0], c[0, 0, 1], c[0, 1, 0], c[0, 1, 1] = 0.0, 1.0, -0.03, 1.08
    c[m - 1] = 1.0
    return np.ascontiguousarray(c)
