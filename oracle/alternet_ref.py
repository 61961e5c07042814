"""CPU restatement of the hybrid conv + window-attention backbone (TEST INFRASTRUCTURE, see oracle/__init__.py).

Follows /root/reference/nets/AlterNet_SwinV2_FAN.py:
  * SwinTransformerBlock (:306-450): attention ONLY (no MLP), x = x + BN(attn(windows(roll(x)))), window sizes
    6/6/6/3, the second block of every pair is shifted by ws//2 with the -100 region mask (:375-397, :420-440);
    dim == dim_out everywhere in AlterNet50, so the 1x1 shortcut branch (:351-356) never exists.
  * AlterNet (:637-751): stem conv3x3 STRIDE 2 + BN + ReLU + MaxPool, four stages of IR BasicBlocks with attention
    pairs inserted by the rule of stack_layers (:685-731), tail bn2 -> ReLU -> Dropout -> AdaptiveAvgPool(6,6)
    -> fc(512*36 -> 512) -> bn3.  AlterNet50 = blocks [3,4,14,4], attention pairs [0,1,4,1], heads (2,4,8,16),
    only constructible at img_size 192.
DropPath(0.1) (:372, :444) and Dropout(0.5) (:667, :745) are identity in eval.  In training the RNG-free fixtures set both to zero; the
*_stochastic fixtures inject portable draws (oracle.recipe.keep_factors / dropout_mask): `keeps` holds one row of per-sample factors
{0, 1/keep_prob} per attention block in network order (timm's drop_path with scale_by_keep, applied to the normalised branch), and
`dropout_mask` is a {0, 1/(1-p)} multiplier in NCHW layout applied after the ReLU of bn2, before the pool and the flatten.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import resnet_ref, swin_ref

ALTER = {"AlterNet50": ((3, 4, 14, 4), (0, 1, 4, 1), (2, 4, 8, 16))}
WINDOWS = (6, 6, 6, 3)


def coords_table(ws):
    r = torch.arange(-(ws - 1), ws, dtype=torch.float32) / (ws - 1) * 8
    t = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    return torch.sign(t) * torch.log2(torch.abs(t) + 1.0) / np.log2(8)


def position_index(ws):
    c = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (ws - 1)
    return rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]


def shift_mask(h, w, ws, shift):
    img = torch.zeros((1, h, w, 1))
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    mw = swin_ref.to_windows(img, ws).view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, -100.0).masked_fill(m == 0, 0.0)


def alter_plan(name, emd_size=512, img=192):
    """[(layer, idx, kind 'basic'|'attn', cin, cout, stride, has_ds, heads, ws, shift, res)]"""
    blocks, blocks2, heads = ALTER[name]
    plan, inplanes = [], 64
    for li, (planes, nb, nb2, hd, ws, stride) in enumerate(zip((64, 128, 256, emd_size), blocks, blocks2, heads, WINDOWS,
                                                              (1, 2, 2, 2)), start=1):
        res = img // (4 * 2 ** (li - 1))
        num = 2 * (nb // 3) + (nb % 3) - 1
        assert 3 * nb2 <= nb
        alt = [False] * num
        for i in range(nb2):
            alt[-2 * i - 1] = True
        idx = 0
        plan.append((li, idx, "basic", inplanes, planes, stride, stride != 1 or inplanes != planes, hd, ws, 0, res))
        idx += 1
        inplanes = planes
        for is_alt in alt:
            if not is_alt:
                plan.append((li, idx, "basic", planes, planes, 1, False, hd, ws, 0, res))
                idx += 1
            else:
                plan.append((li, idx, "attn", planes, planes, 1, False, hd, ws, 0, res))
                plan.append((li, idx + 1, "attn", planes, planes, 1, False, hd, ws, ws // 2, res))
                idx += 2
    return plan


def attn_block_spec(p, c, heads, ws, shift, res):
    t = 2 * ws - 1
    spec = [(p + ".attn_mask", (res // ws * (res // ws), ws * ws, ws * ws), "attn_mask:%d:%d:%d" % (res, ws, shift))] if shift else []
    spec += [(p + ".attn.logit_scale", (heads, 1, 1), "logit_scale"), (p + ".attn.q_bias", (c,), "linear_b"),
             (p + ".attn.v_bias", (c,), "linear_b"),
             (p + ".attn.relative_coords_table", (1, t, t, 2), "coords:%d" % ws),
             (p + ".attn.relative_position_index", (ws * ws, ws * ws), "posidx:%d" % ws),
             (p + ".attn.cpb_mlp.0.weight", (512, 2), "linear_w"), (p + ".attn.cpb_mlp.0.bias", (512,), "linear_b"),
             (p + ".attn.cpb_mlp.2.weight", (heads, 512), "linear_w"), (p + ".attn.qkv.weight", (3 * c, c), "linear_w"),
             (p + ".attn.proj.weight", (c, c), "linear_w"), (p + ".attn.proj.bias", (c,), "linear_b")]
    return spec + resnet_ref._bn_spec(p + ".norm2", c)


def alter_spec(name, emd_size=512, img=192):
    spec = [("conv1.weight", (64, 3, 3, 3), "conv")] + resnet_ref._bn_spec("bn1", 64)
    for li, idx, kind, cin, cout, stride, ds, hd, ws, shift, res in alter_plan(name, emd_size, img):
        p = "layer%d.%d" % (li, idx)
        if kind == "basic":
            spec.append((p + ".conv1.weight", (cin, cin, 3, 3), "conv"))
            spec += resnet_ref._bn_spec(p + ".bn1", cin)
            spec.append((p + ".conv2.weight", (cout, cin, 3, 3), "conv"))
            spec += resnet_ref._bn_spec(p + ".bn2", cout)
            if ds:
                spec.append((p + ".downsample.0.weight", (cout, cin, 1, 1), "conv"))
                spec += resnet_ref._bn_spec(p + ".downsample.1", cout)
        else:
            spec += attn_block_spec(p, cout, hd, ws, shift, res)
    spec += resnet_ref._bn_spec("bn2", emd_size)
    spec += [("fc.weight", (emd_size, emd_size * 36), "linear_w"), ("fc.bias", (emd_size,), "linear_b")]
    spec += resnet_ref._bn_spec("bn3", emd_size)
    return spec


def fill_special(sd, spec):
    for k, shape, kind in spec:
        if kind.startswith("coords:"):
            sd[k] = coords_table(int(kind.split(":")[1]))
        elif kind.startswith("posidx:"):
            sd[k] = position_index(int(kind.split(":")[1]))
        elif kind.startswith("attn_mask:"):
            _, res, ws, shift = kind.split(":")
            sd[k] = shift_mask(int(res), int(res), int(ws), int(shift))
        elif kind == "logit_scale":
            sd[k] = torch.log(10 * torch.ones(shape)) + 0.05 * torch.arange(shape[0], dtype=torch.float32).view(shape)
    return sd


def attn_block(sd, p, x, heads, ws, shift, training, keep=None):
    """x NCHW -> NCHW:  x + BN(attention over (shifted) ws x ws windows); keep [B]: stochastic-depth factor of every sample's branch"""
    b, c, h, w = x.shape
    y = x.permute(0, 2, 3, 1)
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    a = swin_ref.window_attention(sd, p + ".attn", swin_ref.to_windows(y, ws), heads,
                                  mask=sd[p + ".attn_mask"] if shift else None)
    a = swin_ref.from_windows(a, b, h, w, ws)
    if shift:
        a = torch.roll(a, shifts=(shift, shift), dims=(1, 2))
    n = resnet_ref._bn(sd, p + ".norm2", a.permute(0, 3, 1, 2), training)
    if keep is not None:
        n = n * keep.view(-1, 1, 1, 1)
    return x + n


def attn_positions(name, emd_size=512, img=192):
    """indices into alter_plan() of the attention blocks, network order (= the rows of `keeps`)"""
    return [i for i, e in enumerate(alter_plan(name, emd_size, img)) if e[2] == "attn"]


def check_keep_factors(keeps, name, keep_prob, emd_size=512, img=192):
    """the conditions a stored stochastic-depth seed must meet for a fixture to exercise the wiring: enough drops, blocks with none and
    with several, a sample dropped in consecutive blocks, a drop in an attention block that FOLLOWS a conv block's BatchNorm consumer and
    in one that follows another attention block (the two shapes of the reduction handed to the next layer's data-gradient in backward),
    and no block that drops every sample (its BatchNorm gradients would vanish and pin nothing)."""
    plan, pos = alter_plan(name, emd_size, img), attn_positions(name, emd_size, img)
    k = keeps.numpy()
    assert k.shape[0] == len(pos) and set(np.unique(k).tolist()) == {0.0, float(np.float32(1.0) / np.float32(keep_prob))}
    z = k == 0
    assert z.sum() >= 8, z.sum()
    assert (z.sum(1) == 0).any() and (z.sum(1) >= 2).any() and not z.all(1).any()
    runs = [j for j in range(len(pos) - 1) if pos[j + 1] == pos[j] + 1]
    assert any((z[j] & z[j + 1]).any() for j in runs)               # one sample dropped in two attention blocks that are neighbours in the network
    # the attention block in front of a BasicBlock / in front of another attention block (the last of each kind in network order)
    before_basic = [j for j in range(len(pos)) if pos[j] + 1 < len(plan) and plan[pos[j] + 1][2] == "basic"]
    before_attn = [j for j in range(len(pos)) if pos[j] + 1 < len(plan) and plan[pos[j] + 1][2] == "attn"]
    assert z[before_basic[-1]].any() and z[before_attn[-1]].any()


def tail(sd, y, training, dropout_mask=None, kink=0.0):
    """bn2 -> ReLU -> [Dropout as a multiplier, NCHW] -> AdaptiveAvgPool(6,6) -> flatten -> fc -> bn3
    kink != 0 (tools/kink_shift.py only): the ReLU's threshold moved there, values unchanged -- what an implementation whose bn2 output is
    off by `kink` decides differently"""
    y = resnet_ref._bn(sd, "bn2", y, training)
    y = F.relu(y) if kink == 0.0 else y * (y > kink)
    if dropout_mask is not None:
        y = y * dropout_mask
    y = F.adaptive_avg_pool2d(y, (6, 6)).reshape(y.shape[0], -1)
    y = F.linear(y, sd["fc.weight"], sd["fc.bias"])
    return resnet_ref._bn(sd, "bn3", y, training)


def alter_forward(sd, x, name, training, emd_size=512, keeps=None, dropout_mask=None):
    img = x.shape[-1]
    y = F.conv2d(x, sd["conv1.weight"], None, 2, 1)
    y = F.relu(resnet_ref._bn(sd, "bn1", y, training))
    y = F.max_pool2d(y, 3, 2, 1)
    ki = 0
    for li, idx, kind, cin, cout, stride, ds, hd, ws, shift, res in alter_plan(name, emd_size, img):
        p = "layer%d.%d" % (li, idx)
        if kind == "basic":
            y = resnet_ref.basic_block(sd, p, y, stride, ds, training)
        else:
            y = attn_block(sd, p, y, hd, ws, shift, training, keep=None if keeps is None else keeps[ki])
            ki += 1
    assert keeps is None or ki == len(keeps)
    return tail(sd, y, training, dropout_mask)
