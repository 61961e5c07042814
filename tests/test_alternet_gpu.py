"""The HIP AlterNet path (nets.AlterNet_SwinV2_FAN drop-in) against reference-generated fixtures."""
import types

import numpy as np
import pytest
import torch

from oracle import alternet_ref, recipe

pytestmark = pytest.mark.gpu
NOISE = ("proj.bias", "v_bias")


@pytest.mark.parametrize("tag", ["c128_w6", "c512_w3"])
def test_attention_pair_fp32_matches_reference_fixture(golden, tag):
    """(W-MSA, SW-MSA) pair: cyclic roll + region mask + 6x6 / 3x3 windows inside the kernel, fwd + bwd"""
    import nets.AlterNet_SwinV2_FAN as A
    from nets._backbone import BackwardCtx
    g = golden("alternet_pair_" + tag)
    c, heads, ws, res = int(g["c"]), int(g["heads"]), int(g["ws"]), int(g["res"])
    blks = []
    for j, shift in enumerate((0, ws // 2)):
        blk = A.SwinTransformerBlock(c, c, heads=heads, input_resolution=(res, res), window_size=ws, shift_size=shift)
        blk.drop_path_rate = 0.0
        spec = alternet_ref.attn_block_spec("blk", c, heads, ws, shift, res)
        sd = alternet_ref.fill_special(recipe.fill_state(spec, 7000 + 10 * heads + j), spec)
        blk.load_state_dict({k[4:]: v for k, v in sd.items()}, strict=True)
        blks.append(blk.cuda().train())
    x = recipe.normal(7101, (2, c, res, res)).permute(0, 2, 3, 1).contiguous().cuda()
    gy = recipe.normal(7102, (2, c, res, res)).permute(0, 2, 3, 1).contiguous().cuda()
    y0, s0 = A.attn_block_forward(blks[0], x, torch.float32, True, True)
    y1, s1 = A.attn_block_forward(blks[1], y0, torch.float32, True, True)
    params = [p for b in blks for p in b.parameters()]
    bc = BackwardCtx(params, x.device)
    d1 = A.attn_block_backward(blks[1], s1, gy, torch.float32, bc)
    d0 = A.attn_block_backward(blks[0], s0, d1, torch.float32, bc)
    grads = bc.join()
    torch.cuda.synchronize()
    np.testing.assert_allclose(y1.permute(0, 3, 1, 2).cpu().numpy(), g["out"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(d0.permute(0, 3, 1, 2).cpu().numpy(), g["dx"], rtol=2e-3, atol=2e-4)
    for j, blk in enumerate(blks):
        for k, p in blk.named_parameters():
            want = g["b%d.grad.%s" % (j, k)]
            got = grads[p].cpu()
            if want.shape == (10,) and got.numel() != 10:
                np.testing.assert_allclose(recipe.summary(got), want, rtol=5e-3, atol=5e-3 * abs(want[1]) + 1e-4, err_msg=k)
            else:
                np.testing.assert_allclose(got.numpy().reshape(want.shape), want, rtol=5e-3,
                                           atol=(2e-3 if k.endswith(NOISE) else 5e-3 * np.abs(want).max() + 1e-5), err_msg=k)


def test_alternet50_fp32_eval(golden):
    import nets.AlterNet_SwinV2_FAN as A
    g = golden("alternet50_b2_eval")
    spec = alternet_ref.alter_spec("AlterNet50")
    sd = alternet_ref.fill_special(recipe.fill_state(spec, 7300), spec)
    net = A.Encoder(types.SimpleNamespace(network="AlterNet50", emd_size=512, img_size=192, frhip_dtype="fp32"))
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    with torch.no_grad():
        y = net(recipe.images(7301, 2, 192, 192).cuda())
    np.testing.assert_allclose(y.cpu().numpy(), g["out"], rtol=1e-3, atol=3e-4)



def _alternet50(dtype, seed):
    import nets.AlterNet_SwinV2_FAN as A
    spec = alternet_ref.alter_spec("AlterNet50")
    sd = alternet_ref.fill_special(recipe.fill_state(spec, seed), spec)
    net = A.Encoder(types.SimpleNamespace(network="AlterNet50", emd_size=512, img_size=192, frhip_dtype=dtype))
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def test_alternet50_whole_net_training_mode_fp32_matches_reference_fixture(golden):
    """BASELINE cfg 5's network (/root/reference/nets/AlterNet_SwinV2_FAN.py:637-751) in training mode against the real reference, batch 8 at
    192 x 192: stride-2 stem (im2col route), conv <-> (W-MSA, SW-MSA) interleave, bn2 -> ReLU -> Dropout(p = 0) -> AAP(6,6) -> fc -> bn3."""
    from wholenet import check_whole_net_train, whole_net_train_on_gpu
    g = golden("alternet50_b8_train")
    grads, out, bufs = whole_net_train_on_gpu(_alternet50("fp32", int(g["seed"])), g, 192, 192)
    check_whole_net_train(g, grads, out, bufs, rtol=2e-3, noise=("fc.bias",), kink_rtol=5e-2,
                          kink_free=("fc.", "bn3.", "bn2.", "layer4.3.norm2.", "layer4.3.attn.proj."))


def test_alternet50_bf16_training_step_tracks_the_reference_fixture(golden):
    """bf16 MFMA mode on the fixture's inputs.  This randomly initialised 50-block network at batch 8 amplifies bf16 STORAGE rounding to a
    20 % embedding error in a plain PyTorch emulation with no HIP code (wholenet.alternet50_bf16_storage_emulation: 0.197); the HIP path must
    not be worse than that by more than 15 %, and its large gradients must point the reference's way."""
    from wholenet import alternet50_bf16_storage_emulation, whole_net_train_on_gpu
    g = golden("alternet50_b8_train")
    grads, out, _ = whole_net_train_on_gpu(_alternet50("bf16", int(g["seed"])), g, 192, 192)
    assert np.isfinite(out).all() and all(torch.isfinite(v).all() for v in grads.values())
    emu = alternet50_bf16_storage_emulation(g)
    err = float(np.linalg.norm(out - g["out"]) / np.linalg.norm(g["out"]))
    assert err <= 1.15 * emu + 5e-3, (err, emu)
    for k in [k[6:] for k in g if k.startswith("gfull.")]:
        want = g["gfull." + k].reshape(-1).astype(np.float64)
        got = grads[k].numpy().reshape(-1).astype(np.float64)
        if want.size >= 16384:              # (the 2 048-element position-bias MLP gradients of stage 2 sit at 0.79 after 40 bf16 blocks)
            cos = float(got @ want / (np.linalg.norm(got) * np.linalg.norm(want)))
            assert cos >= 0.80, (k, cos)


def test_stochastic_depth_reductions_fused_into_the_producing_data_gradient(monkeypatch):
    """AlterNet50 in training mode WITH stochastic depth (drop_path 0.1, the reference default): the BatchNorm-backward sums of an attention
    block's norm2 ride in the data-gradient that produces its incoming gradient (frhip_conv_dgrad_fused_rs) instead of a pass of their own --
    every parameter gradient must equal the unfused route's on the same per-sample keep draws."""
    import nets.AlterNet_SwinV2_FAN as A
    x = recipe.images(7501, 8, 192, 192).cuda()
    gy = recipe.normal(7502, (8, 512), 0.05).cuda()
    res = []
    for fused in (True, False):
        monkeypatch.setattr(A, "_FUSE_BNRED_RS", fused)
        net = _alternet50("fp32", 7500).train()
        net.dropout.p = 0.0
        torch.manual_seed(7503)                      # the keep masks come from torch's device generator
        y = net(x)
        y.backward(gy)
        torch.cuda.synchronize()
        res.append((y.detach().float().cpu(), {k: p.grad.float().cpu() for k, p in net.named_parameters()}))
    (ya, ga), (yb, gb) = res
    assert torch.equal(ya, yb)                       # same forward, same keeps
    dropped = 0
    for k in ga:
        if k.endswith(NOISE) or k == "fc.bias":          # analytically-zero gradients: round-off only
            continue
        a, b = ga[k].double(), gb[k].double()
        denom = float(b.norm()) + 1e-12
        assert float((a - b).norm()) <= 1e-3 * denom + 1e-7, (k, float((a - b).norm()) / denom)
        dropped += 1
    assert dropped > 150


KINK_FREE = ("fc.", "bn3.", "bn2.", "layer4.3.norm2.", "layer4.3.attn.proj.")


@pytest.mark.parametrize("fused", [True, False])
def test_alternet50_whole_net_stochastic_fp32_matches_reference_fixture(golden, monkeypatch, fused):
    """The network as it SHIPS -- DropPath(0.1) in all twelve attention blocks, Dropout(0.5) in the tail -- against the real reference on
    the same draws (fixture alternet50_b8_train_stochastic; wholenet.inject_draws hands the product the rows / the mask the reference was
    given and asserts that every block and the tail consumed theirs).  This holds to the reference what only compared the product with
    itself before: the factor in forward (frhip_bn_apply_rs), in norm2's backward, in the reduction handed to the next layer's
    data-gradient (both shapes of `nxt`: a BasicBlock and an attention block behind a dropping block; fused and unfused), the row order,
    the 1/keep, the dropout mask's NHWC layout against the reference's NCHW, and its place behind the ReLU mask in tail_backward.
    Tolerances: those of the RNG-free test.  kink_rtol re-measured for this input and these masks on the oracle (tools/kink_shift.py):
    10 of the 147 456 pre-ReLU values of bn2 lie within 1e-4 of zero and the dropout mask (seed chosen for it, tools/make_golden.py)
    zeroes all ten, so shifting the kink by 1e-4 flips nothing and moves nothing (0.0 on every tensor); by 2e-4: 2 flips,
    layer4.3.attn.qkv.weight moves by 7.9e-3 in the check's terms, 1.6e-2 at most on every stored element upstream but one
    (layer4.2.attn.proj.weight, 8.2e-2).  The bound stays the 5e-2 of the RNG-free test, the tail's own tensors at rtol."""
    import nets.AlterNet_SwinV2_FAN as A
    from wholenet import check_whole_net_train, stochastic_draws, whole_net_train_on_gpu
    monkeypatch.setattr(A, "_FUSE_BNRED_RS", fused)
    g = golden("alternet50_b8_train_stochastic")
    keeps, mask = stochastic_draws(g)
    net = _alternet50("fp32", int(g["seed"]))
    assert net.dropout.p == float(g["dropout_p"]) and {m.drop_path_rate for m in net.modules() if hasattr(m, "drop_path_rate")} == {float(g["drop_path_rate"])}
    grads, out, bufs = whole_net_train_on_gpu(net, g, 192, 192, keeps=keeps, dropout_mask=mask)
    check_whole_net_train(g, grads, out, bufs, rtol=2e-3, noise=("fc.bias",), kink_rtol=5e-2, kink_free=KINK_FREE)


def test_alternet50_bf16_stochastic_training_step_tracks_the_reference_fixture(golden):
    """bf16 MFMA mode with both random paths on, same injected draws, under the rule of the RNG-free bf16 test: the embedding error is at
    most 1.15 x the error of the mask-aware bf16-STORAGE emulation of the oracle (wholenet.alternet50_bf16_storage_emulation with the
    same rows and mask: 0.171 on this input) + 5e-3, and the large gradients keep a cosine of 0.80 with the reference's."""
    from wholenet import alternet50_bf16_storage_emulation, stochastic_draws, whole_net_train_on_gpu
    g = golden("alternet50_b8_train_stochastic")
    keeps, mask = stochastic_draws(g)
    grads, out, _ = whole_net_train_on_gpu(_alternet50("bf16", int(g["seed"])), g, 192, 192, keeps=keeps, dropout_mask=mask)
    assert np.isfinite(out).all() and all(torch.isfinite(v).all() for v in grads.values())
    emu = alternet50_bf16_storage_emulation(g, keeps, mask)
    err = float(np.linalg.norm(out - g["out"]) / np.linalg.norm(g["out"]))
    print("bf16 stochastic: err %.4f emulation %.4f bound %.4f" % (err, emu, 1.15 * emu + 5e-3))
    assert err <= 1.15 * emu + 5e-3, (err, emu)
    big = [k[6:] for k in g if k.startswith("gfull.") and g[k].size >= 16384]
    assert len(big) >= 3
    for k in big:
        want = g["gfull." + k].reshape(-1).astype(np.float64)
        got = grads[k].numpy().reshape(-1).astype(np.float64)
        cos = float(got @ want / (np.linalg.norm(got) * np.linalg.norm(want)))
        print("bf16 stochastic: cos %.4f %s" % (cos, k))
        assert cos >= 0.80, (k, cos)


def _captured_draws(net, x, seed):
    """one training forward of the product on ITS OWN draws (nothing injected): what every attention block received as `keep`, in
    network order, and the tail's mask"""
    import nets.AlterNet_SwinV2_FAN as A
    from frhip import ops
    orig_block, orig_mask = A.attn_block_forward, ops.dropout_mask
    rows, masks = [], []

    def block(blk, x_, dt, training, save, *a, **kw):
        out, s = orig_block(blk, x_, dt, training, save, *a, **kw)
        rows.append(s.keep if s is not None else kw.get("keep"))
        return out, s

    def mask(*a, **kw):
        masks.append(orig_mask(*a, **kw))
        return masks[-1]

    A.attn_block_forward, ops.dropout_mask = block, mask
    try:
        if seed is not None:
            torch.manual_seed(seed)              # the device generator: the stochastic-depth factors
            ops.seed_dropout(seed)               # the stream of the dropout kernel's seeds (frhip.ops._drop_generator follows
                                                 # torch.manual_seed only when the seed VALUE changes; this pins it outright)
        y = net(x)
        torch.cuda.synchronize()
    finally:
        A.attn_block_forward, ops.dropout_mask = orig_block, orig_mask
    return rows, masks, y


def test_product_draws_have_the_reference_statistics():
    """The product's OWN stochastic-depth and dropout draws (nothing injected, capture only), B = 64: every attention block gets a row of
    exactly {0, 1/0.9}; over n = 5 forwards x 12 blocks x 64 samples = 3 840 factors the kept fraction is within 5 sigma of 0.9
    (sigma = sqrt(0.9 x 0.1 / n)); rows of different blocks and of different forwards differ; torch.manual_seed reproduces them; the
    tail's mask is {0, 2} with half of it kept (n = 64 x 18 432: 5 sigma = 2.3e-3), differs between forwards and is reproduced by
    frhip.ops.seed_dropout."""
    net = _alternet50("bf16", 7700).train()                      # (the draws do not depend on the compute type; bf16 is the quicker pass)
    x = recipe.images(7701, 64, 192, 192).cuda()
    runs = []
    for it in range(5):
        rows, masks, _ = _captured_draws(net, x, 7702 if it == 0 else None)
        assert len(rows) == 12 and all(r is not None and tuple(r.shape) == (64,) for r in rows) and len(masks) == 1
        if all(r._base is not None and r._base is rows[0]._base for r in rows):        # drawn as one [blocks, B] tensor: block i reads row i
            assert [r.storage_offset() for r in rows] == [64 * i for i in range(12)]
        runs.append((torch.stack(rows).cpu(), masks[0].float().cpu()))
    f = torch.stack([r for r, _ in runs])                       # [5, 12, 64]
    n = f.numel()
    assert n >= 3000
    vals = torch.unique(f).tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1.0 / 0.9) <= 2.0 ** -23 * 1.2, vals      # one float32 rounding of 1/0.9
    kept = float((f != 0).float().mean())
    assert abs(kept - 0.9) <= 5 * (0.09 / n) ** 0.5, kept
    flat = f.view(-1, 64)
    assert len({tuple(r.tolist()) for r in flat}) > 0.9 * flat.shape[0]              # not one row broadcast to the blocks / replayed per forward
    m = runs[0][1]
    assert set(torch.unique(m).tolist()) == {0.0, 2.0} and tuple(m.shape) == (64, 6, 6, 512)
    assert abs(float((m != 0).float().mean()) - 0.5) <= 5 * (0.25 / m.numel()) ** 0.5
    assert not torch.equal(runs[0][1], runs[1][1])
    rows, masks, _ = _captured_draws(net, x, 7702)              # the same seed: the same draws
    assert torch.equal(torch.stack(rows).cpu(), runs[0][0]) and torch.equal(masks[0].float().cpu(), runs[0][1])


def test_eval_mode_draws_nothing_and_equals_the_rate_zero_network():
    """eval mode: no factor, no mask, the device generator untouched, and the outputs of the shipped configuration (rate 0.1, p 0.5)
    equal those of a drop_path_rate = 0, p = 0 copy bit for bit"""
    x = recipe.images(7711, 4, 192, 192).cuda()
    net = _alternet50("fp32", 7710).eval()
    ref = _alternet50("fp32", 7710).eval()
    ref.dropout.p = 0.0
    for m in ref.modules():
        if hasattr(m, "drop_path_rate"):
            m.drop_path_rate = 0.0
    torch.manual_seed(7712)
    before = torch.cuda.get_rng_state()
    with torch.no_grad():
        rows, masks, y = _captured_draws(net, x, None)
        y_ref = ref(x)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    assert len(rows) == 12 and all(r is None for r in rows) and masks == []
    assert torch.equal(y, y_ref)
    # ... and on the differentiable eval path (input gradients), which saves what backward reads: no factor saved either
    xg = x.clone().requires_grad_(True)
    rows, masks, yg = _captured_draws(net, xg, None)
    assert all(r is None for r in rows) and masks == [] and torch.equal(torch.cuda.get_rng_state(), before)
    assert torch.equal(yg.detach(), ref(x.clone().requires_grad_(True)).detach())
