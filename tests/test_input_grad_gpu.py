"""Input-image gradients and eval-mode backward of the HIP backbones: x.grad (and, in eval mode, every parameter gradient) against float64
CPU autograd through the oracle restatements; the stem image-gradient kernels at bench shape against a float64 restatement; the
input-gradient-only backward; the default training path unchanged."""
import contextlib
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import alternet_ref, recipe, resnet_ref, swin_ref
from poison import PATTERNS, poisoned_empty

pytestmark = pytest.mark.gpu

WGRAD_OPS = ("conv_wgrad", "conv_wgrad_bnrelu", "conv_wgrad_chain", "gemm_tn", "stem_gram", "stem_bwd", "unpack_stem_grad",
             "fc_unpermute_grad", "colsum_accumulate")
DX_OPS = ("stem_dx", "stem_dx_s2", "bn_eval_state")


@contextlib.contextmanager
def recorded(names):
    """counts the calls of the named frhip.ops functions (the nets call them through the module)"""
    from frhip import ops
    calls = {n: 0 for n in names}
    saved = {n: getattr(ops, n) for n in names}

    def wrap(n, fn):
        def w(*a, **k):
            calls[n] += 1
            return fn(*a, **k)
        return w
    for n in names:
        setattr(ops, n, wrap(n, saved[n]))
    try:
        yield calls
    finally:
        for n, fn in saved.items():
            setattr(ops, n, fn)


def rel_l2(got, want):
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


def oracle_grads(fwd, sd, x, g, training, dtype=torch.float64):
    """CPU autograd of the oracle in `dtype`: (x.grad, {param: grad}, state dict after the pass), in float64"""
    sdq = {k: (v.to(dtype).clone() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    names = [k for k in resnet_ref.trainable_names(sdq) if sdq[k].is_floating_point()]
    for k in names:
        sdq[k].requires_grad_(True)
    xq = x.to(dtype).clone().requires_grad_(True)
    y = fwd(sdq, xq, training)
    y.backward(g.to(dtype))
    return xq.grad.double(), {k: None if sdq[k].grad is None else sdq[k].grad.double() for k in names}, sdq


class Oracle:
    """float64 gradients, and the distance plain fp32 autograd of the same restatement lands from them.  These randomly initialised nets at
    batch 2 - 4 are kink-sensitive (ReLU / max-pool decisions flip under fp32 rounding, amplified by training-mode BatchNorm over a few
    samples): fp32 PyTorch itself is 1e-3 (eval) to 4e-3 (training, ResNet18) away from float64 in x.grad.  A gradient passes when it is
    within 1e-3 of float64, or no more than 3x as far as fp32 PyTorch is."""

    def __init__(self, fwd, sd, x, g, training):
        self.dx, self.p, self.sd = oracle_grads(fwd, sd, x, g, training)
        self.dx32, self.p32, _ = oracle_grads(fwd, sd, x, g, training, torch.float32)

    def bound(self, got, want, want32, floor=1e-3):
        return max(floor, 3.0 * rel_l2(want32, want))


def check_x_grad(got, orc):
    assert got is not None and got.dtype == torch.float32 and tuple(got.shape) == tuple(orc.dx.shape)
    got = got.detach().cpu().double()
    err, bound = rel_l2(got, orc.dx), orc.bound(got, orc.dx, orc.dx32)
    assert err < bound, (err, bound)
    cos = float((got.reshape(-1) @ orc.dx.reshape(-1)) / (got.norm() * orc.dx.norm()))
    assert cos > 1 - bound, cos


def check_param_grads(net, orc):
    for k, p in net.named_parameters():
        w = orc.p[k]
        if w is None or float(w.norm()) == 0.0:
            continue
        assert p.grad is not None, k
        err, bound = rel_l2(p.grad.detach().cpu(), w), orc.bound(None, w, orc.p32[k], 2e-3)
        assert err < bound, (k, err, bound)


# ------------------------------------------------------------------------------------------------- ResNet18
def _resnet(name, dtype, seed, **kw):
    import nets.resnet as R
    net = R.Encoder(types.SimpleNamespace(network=name, emd_size=512, frhip_dtype=dtype, **kw))
    sd = recipe.fill_state(resnet_ref.resnet_spec(resnet_ref.BLOCKS[name]), seed)
    net.load_state_dict(sd, strict=True)
    return net.cuda(), sd


def _resnet_fwd(blocks):
    return lambda sd, x, training: resnet_ref.resnet_forward(sd, x, blocks, training)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_resnet18_fp32_input_gradient_matches_oracle(mode):
    net, sd = _resnet("ResNet18", "fp32", 8100)
    net.train(mode == "train")
    x = recipe.images(8101, 4)
    g = recipe.normal(8102, (4, 512), 0.05)
    buffers = {k: b.clone() for k, b in net.named_buffers()}
    xg = x.cuda().requires_grad_(True)
    net(xg).backward(g.cuda())
    orc = Oracle(_resnet_fwd(resnet_ref.BLOCKS["ResNet18"]), sd, x, g, mode == "train")
    check_x_grad(xg.grad, orc)
    if mode == "eval":
        check_param_grads(net, orc)
        for k, b in net.named_buffers():
            assert torch.equal(b, buffers[k]), k                          # running statistics and counters untouched
    else:
        for k, b in net.named_buffers():
            if b.is_floating_point():
                assert rel_l2(b.cpu(), orc.sd[k].detach()) < 1e-4, k


def test_resnet18_training_parameter_gradients_do_not_depend_on_x_requires_grad():
    outs = []
    for want_x in (False, True):
        net, _ = _resnet("ResNet18", "fp32", 8200)
        net.train()
        x = recipe.images(8201, 4).cuda().requires_grad_(want_x)
        net(x).backward(recipe.normal(8202, (4, 512), 0.05).cuda())
        assert (x.grad is not None) == want_x
        outs.append({k: p.grad.clone() for k, p in net.named_parameters()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_resnet18_input_only_backward(mode):
    """net.requires_grad_(False): x.grad bit-identical to the full backward's, no parameter gradient, no weight-gradient op called"""
    net, _ = _resnet("ResNet18", "fp32", 8300)
    net.train(mode == "train")
    x = recipe.images(8301, 4).cuda()
    g = recipe.normal(8302, (4, 512), 0.05).cuda()
    xf = x.clone().requires_grad_(True)
    net(xf).backward(g)
    net, _ = _resnet("ResNet18", "fp32", 8300)          # same weights, same running statistics before the pass
    net.train(mode == "train")
    net.requires_grad_(False)
    xi = x.clone().requires_grad_(True)
    with recorded(WGRAD_OPS) as calls:
        net(xi).backward(g)
    torch.cuda.synchronize()
    assert not any(calls.values()), calls
    assert all(p.grad is None for p in net.parameters())
    assert torch.equal(xi.grad, xf.grad)


# ------------------------------------------------------------------------------------------------- Swin18 / AlterNet50
def _swin18():
    import nets.SwinV2 as S
    net = S.Encoder(types.SimpleNamespace(network="Swin18", emd_size=512, frhip_dtype="fp32"))
    spec = swin_ref.swin_spec("Swin18")
    sd = swin_ref.fill_special(recipe.fill_state(spec, 8400), spec)
    net.load_state_dict(sd, strict=True)
    net.dropout.p = 0.0
    return net.cuda(), sd


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_swin18_fp32_input_gradient_matches_oracle(mode):
    net, sd = _swin18()
    net.train(mode == "train")
    x = recipe.images(8401, 2)
    g = recipe.normal(8402, (2, 512), 0.05)
    xg = x.cuda().requires_grad_(True)
    net(xg).backward(g.cuda())
    orc = Oracle(lambda s, xx, t: swin_ref.swin_forward(s, xx, "Swin18", t), sd, x, g, mode == "train")
    check_x_grad(xg.grad, orc)
    if mode == "eval":
        check_param_grads(net, orc)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_alternet50_fp32_input_gradient_matches_oracle(mode):
    import nets.AlterNet_SwinV2_FAN as A
    spec = alternet_ref.alter_spec("AlterNet50")
    sd = alternet_ref.fill_special(recipe.fill_state(spec, 8500), spec)
    net = A.Encoder(types.SimpleNamespace(network="AlterNet50", emd_size=512, img_size=192, frhip_dtype="fp32"))
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    for blk in net.modules():
        if isinstance(blk, A.SwinTransformerBlock):
            blk.drop_path_rate = 0.0                    # stochastic depth off (the oracle has none)
    net.dropout.p = 0.0
    net.train(mode == "train")
    x = recipe.images(8501, 2, 192, 192)
    g = recipe.normal(8502, (2, 512), 0.05)
    xg = x.cuda().requires_grad_(True)
    net(xg).backward(g.cuda())
    orc = Oracle(lambda s, xx, t: alternet_ref.alter_forward(s, xx, "AlterNet50", t), sd, x, g, mode == "train")
    check_x_grad(xg.grad, orc)
    if mode == "eval":
        check_param_grads(net, orc)


# ------------------------------------------------------------------------------------------------- the kernels at bench shape
def _round(t, dt):
    return t.to(dt).double()


def _stem_case(b, h, w, dt, seed, eval_coef):
    from frhip import ops
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(b, 3, h, w, device="cuda", generator=gen)
    w27 = torch.randn(64, 27, device="cuda", generator=gen) * 0.2
    wp = ops.pack_stem(w27, dt, kp=32)
    gamma = torch.rand(64, device="cuda", generator=gen) + 0.5
    beta = torch.randn(64, device="cuda", generator=gen) * 0.3
    rm = torch.randn(64, device="cuda", generator=gen) * 0.1
    rv = torch.rand(64, device="cuda", generator=gen) + 0.5
    st = ops.bn_eval_affine(gamma, beta, rm, rv)
    pooled, arg = ops.stem_fwd(x, wp, st)
    dpool = (torch.randn(pooled.shape, device="cuda", generator=gen) * 0.1).to(dt)
    coef = torch.randn(3, 64, device="cuda", generator=gen) * 0.3
    if eval_coef:
        coef[1:] = 0.0
    return x, w27, wp, pooled, arg, dpool, coef


def _stem_dx_ref(x, w27, pooled, arg, dpool, coef, dt):
    """float64 restatement: d routed through the kernel's own arg-max bytes, masked by pooled > 0; dy0 = ca d + cb y + cc on the image,
    rounded to the storage dtype as the kernel keeps it; dx = conv^T(dy0)"""
    b, _, h, w = x.shape
    hp, wq = pooled.shape[1:3]
    wt = _round(w27, dt).view(64, 3, 3, 3).permute(0, 3, 1, 2)            # [k][fr][fs][c] -> [k][c][fr][fs]
    y = F.conv2d(_round(x, dt), wt, None, 1, 1)
    d = dpool.double() * (pooled > 0)
    a = arg.long()
    ph = torch.arange(hp, device=x.device).view(1, hp, 1, 1)
    pw = torch.arange(wq, device=x.device).view(1, 1, wq, 1)
    hh = 2 * ph - 1 + a // 3 + 1                                            # +1: into a map padded by one pixel on each side
    ww = 2 * pw - 1 + a % 3 + 1
    bb = torch.arange(b, device=x.device).view(b, 1, 1, 1).expand_as(a)
    kk = torch.arange(64, device=x.device).view(1, 1, 1, 64).expand_as(a)
    dmap = torch.zeros(b, 64, h + 2, w + 2, dtype=torch.float64, device=x.device)
    dmap.index_put_((bb.reshape(-1), kk.reshape(-1), hh.reshape(-1), ww.reshape(-1)), d.reshape(-1), accumulate=True)
    dmap = dmap[:, :, 1:h + 1, 1:w + 1]
    ca, cb, cc = (coef[i].double().view(1, 64, 1, 1) for i in range(3))
    dy0 = _round(ca * dmap + cb * y + cc, dt)
    return F.conv_transpose2d(dy0, wt, None, 1, 1)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("coef_mode", ["train", "eval"])
@pytest.mark.parametrize("shape", [(512, 112, 112), (3, 37, 53)], ids=["bench", "ragged"])
def test_stem_dx_stride1_matches_float64(dt, coef_mode, shape):
    from frhip import ops
    x, w27, wp, pooled, arg, dpool, coef = _stem_case(*shape, dt, 8600, coef_mode == "eval")
    dx = ops.stem_dx(x, wp, dpool, arg, pooled, coef, eval_mode=coef_mode == "eval")
    want = _stem_dx_ref(x, w27, pooled, arg, dpool, coef, dt)
    tol = 2e-3 if dt == torch.bfloat16 else 1e-5
    assert rel_l2(dx, want) < tol, rel_l2(dx, want)
    err = (dx.double() - want).abs().max().item()
    assert err < 50 * tol * float(want.pow(2).mean().sqrt()), err
    assert torch.equal(dx, ops.stem_dx(x, wp, dpool, arg, pooled, coef, eval_mode=coef_mode == "eval"))
    for pat in PATTERNS:
        with poisoned_empty(pat):
            again = ops.stem_dx(x, wp, dpool, arg, pooled, coef, eval_mode=coef_mode == "eval")
        assert torch.equal(dx, again), pat


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(256, 192, 192), (3, 37, 52)], ids=["bench", "ragged"])
def test_stem_dx_stride2_matches_float64(dt, shape):
    from frhip import ops
    b, h, w = shape
    gen = torch.Generator(device="cuda").manual_seed(8700)
    w27 = torch.randn(64, 27, device="cuda", generator=gen) * 0.2
    wp = ops.pack_stem(w27, dt)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy0 = (torch.randn(b, ho, wo, 64, device="cuda", generator=gen) * 0.1).to(dt)
    dx = ops.stem_dx_s2(dy0, wp, h, w)
    wt = _round(w27, dt).view(64, 3, 3, 3).permute(0, 3, 1, 2)
    want = F.conv_transpose2d(dy0.double().permute(0, 3, 1, 2), wt, None, 2, 1, output_padding=(h - (2 * ho - 1), w - (2 * wo - 1)))
    assert tuple(want.shape) == (b, 3, h, w)
    assert rel_l2(dx, want) < 2e-6, rel_l2(dx, want)
    assert torch.equal(dx, ops.stem_dx_s2(dy0, wp, h, w))
    for pat in PATTERNS:
        with poisoned_empty(pat):
            again = ops.stem_dx_s2(dy0, wp, h, w)
        assert torch.equal(dx, again), pat


# ------------------------------------------------------------------------------------------------- the default path / model level
def test_resnet50_bf16_training_step_without_input_gradient_calls_no_image_gradient_op():
    net, _ = _resnet("ResNet50", "bf16", 8800)
    net.train()
    x = recipe.images(8801, 8).cuda()
    with recorded(DX_OPS + ("stem_bwd", "stem_gram")) as calls:
        net(x).backward(recipe.normal(8802, (8, 512), 0.05).cuda())
        torch.cuda.synchronize()
    assert all(calls[n] == 0 for n in DX_OPS), calls
    assert calls["stem_bwd"] == 1 and calls["stem_gram"] == 1, calls
    assert all(p.grad is not None for p in net.parameters())


def test_resnet50_bf16_fgsm_step_on_an_eval_model_lowers_the_loss():
    """one FGSM step x -> x - eps sign(grad) on 1 - cos(emb, target), the encoder of a Model in eval mode, bench batch"""
    import os
    import tempfile

    import torch.distributed as dist
    from model.FR_PartialFC import Model
    own_pg = not dist.is_initialized()
    if own_pg:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(tempfile.mkdtemp(), "pg"), rank=0, world_size=1)
    try:
        conf = types.SimpleNamespace(network="ResNet50", emd_size=512, img_size=112, local_rank=0, world_size=1, sample_rate=1.0,
                                     mixed_precision=False, loss_s=30.0, loss_m=0.35, n_classes=256, optimizer="SGD", lr=0.1, wd=5e-4,
                                     mom=0.9, loss="PartialFC", lr_scheduler=None, frhip_dtype="bf16", ckpt_path=None)
        model = Model(conf, None, "train")
        enc = model.encoder
        enc.eval()
        b = 512
        x = recipe.images(8901, b).cuda()
        target = F.normalize(recipe.normal(8902, (b, 512)).cuda(), dim=1)

        def loss_of(img):
            return (1.0 - F.cosine_similarity(enc(img), target, dim=1)).mean()
        xg = x.clone().requires_grad_(True)
        loss = loss_of(xg)
        loss.backward()
        assert xg.grad is not None and torch.isfinite(xg.grad).all() and float(xg.grad.abs().max()) > 0
        with torch.no_grad():
            after = loss_of(x - 2.0 / 255 * xg.grad.sign())
        assert float(after) < float(loss.detach()), (float(after), float(loss.detach()))
    finally:
        if own_pg:
            dist.destroy_process_group()
