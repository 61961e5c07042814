"""Shared by the oracle (CPU) and the HIP (GPU) whole-network training-mode parity tests (fixtures swin34_b8_train, alternet50_b8_train
and their siblings with the random paths on: alternet50_b8_train_stochastic, swin34_b8_train_dropout)."""
import contextlib
import itertools

import numpy as np
import torch

from oracle import recipe

NOISE_TAILS = ("proj.bias", "fc2.bias", "v_bias")


def check_whole_net_train(g, grads, out, running, rtol=5e-3, noise=(), kink_rtol=None, kink_free=()):
    """shared by the oracle (CPU) and the HIP (GPU) whole-network training-mode tests: embeddings, a probe of EVERY parameter gradient
    (sum, l2, 256 elements at portable positions -- a layout permutation cannot pass), full tensors where the fixture holds them, running
    statistics.  Element tolerance = rtol of the value + 2 rtol x the tensor's rms (fp32 summation order through 30-50 BatchNorm'd blocks).

    kink_rtol: AlterNet's tail is bn2 -> ReLU -> fc, and of its 147 456 pre-ReLU values seven lie within 1e-4 of zero on the fixture's input.
    An implementation whose bn2 output differs from the reference's by 1e-4 (fp32 round-off after 50 blocks) takes the other side of the kink
    for a few of them, which moves EVERY upstream gradient by about 1.4 % of its rms -- measured on the oracle by shifting the kink by 1e-4:
    5 elements flip, layer4.3.attn.qkv.weight moves by 1.40e-2 rms (the HIP fp32 path: 1.39e-2), the tail's own gradients (fc, bn3, bn2,
    layer4.3's proj / norm2) by < 3e-4.  So: the tensors named by `kink_free` prefixes are held to rtol, everything upstream of the kink to
    kink_rtol -- still 30x below what any indexing / layout defect produces (an error of the order of the rms itself)."""
    np.testing.assert_allclose(out, g["out"], rtol=rtol, atol=rtol * float(np.abs(g["out"]).max()))

    def tol_of(k):
        return rtol if (kink_rtol is None or k.startswith(tuple(kink_free))) else kink_rtol

    for key in [k for k in g if k.startswith("gprobe.")]:
        k = key[7:]
        want = g[key]
        got = recipe.probe(grads[k])
        rms = want[1] / max(1.0, float(grads[k].numel())) ** 0.5
        if k.endswith(NOISE_TAILS) or k in noise or rms < 1e-7:           # analytically-zero gradients (a shift in front of a training-mode BatchNorm): size only
            assert np.abs(got[2:]).max() <= 1e-3 + 50 * np.abs(want[2:]).max(), k
            continue
        t = tol_of(k)
        np.testing.assert_allclose(got[1], want[1], rtol=t if grads[k].numel() < 1024 else max(rtol, 0.2 * t), atol=1e-7, err_msg=k + " (l2)")
        np.testing.assert_allclose(got[2:], want[2:], rtol=t, atol=2 * t * rms + 1e-8, err_msg=k)
    for key in [k for k in g if k.startswith("gfull.")]:
        k = key[6:]
        want = g[key]
        rms = float(np.sqrt((want.astype(np.float64) ** 2).mean()))
        t = tol_of(k)
        np.testing.assert_allclose(grads[k].numpy().reshape(want.shape), want, rtol=t, atol=2 * t * rms + 1e-8, err_msg=k + " (full)")
    want = g["gprobe16k.fc.weight"]
    np.testing.assert_allclose(recipe.probe(grads["fc.weight"], 16384)[2:], want[2:], rtol=rtol, atol=2 * rtol * want[1] / grads["fc.weight"].numel() ** 0.5)
    for key in [k for k in g if k.startswith("after.")]:
        np.testing.assert_allclose(recipe.probe(running[key[6:]].float()), g[key], rtol=1e-3, atol=1e-5, err_msg=key)


def stochastic_draws(g, step=0):
    """the injected draws of a *_stochastic / *_dropout fixture, regenerated from its stored seeds: (keeps [blocks, B] or None, dropout
    mask NCHW).  Asserts what tools/make_golden.py asserted when it chose the seeds (oracle.alternet_ref.check_keep_factors)."""
    from oracle import alternet_ref
    b = int(g["batch"]) if "batch" in g else int(g["B"])
    keeps = None
    if "keep_seed" in g:
        kp = 1.0 - float(g["drop_path_rate"])
        keeps = recipe.keep_factors(int(g["keep_seed"]) + step, len(alternet_ref.attn_positions("AlterNet50")), b, kp)
        alternet_ref.check_keep_factors(keeps, "AlterNet50", kp)
    p = float(g["dropout_p"])
    mask = recipe.dropout_mask(int(g["dropout_seed"]) + step, (b, 512, 6, 6) if keeps is not None else (b, 512, 7, 7), p)
    assert set(np.unique(mask.numpy()).tolist()) == {0.0, 1.0 / (1.0 - p)} and abs(float((mask == 0).float().mean()) - p) < 0.02
    return keeps, mask


def alternet50_bf16_storage_emulation(g, keeps=None, dropout_mask=None):
    """relative l2 error of the training-mode embeddings when the ORACLE keeps every activation and convolution weight in bf16 between
    fp32-accumulating ops (oracle.resnet_ref.storage_cast; attention blocks: block output rounded) -- what any bf16-storage
    implementation of the network has by construction, no HIP code involved.  Measured 0.197 on the fixture's input.
    keeps / dropout_mask: the injected draws of alternet50_b8_train_stochastic (both exact in bf16: 0, 1/0.9 rounded once, 2)."""
    import torch.nn.functional as F
    from oracle import alternet_ref, resnet_ref
    name = "AlterNet50"
    spec = alternet_ref.alter_spec(name)
    seed = int(g["seed"])
    sd = alternet_ref.fill_special(recipe.fill_state(spec, seed), spec)
    q = resnet_ref.storage_cast(torch.bfloat16)
    rows = iter(keeps) if keeps is not None else itertools.repeat(None)
    with torch.no_grad():
        y = q(F.conv2d(q(recipe.images(seed + 1, int(g["batch"]), 192, 192)), q(sd["conv1.weight"]), None, 2, 1))
        y = q(F.max_pool2d(F.relu(resnet_ref._bn(sd, "bn1", y, True)), 3, 2, 1))
        for li, idx, kind, cin, cout, stride, ds, hd, ws, shift, res in alternet_ref.alter_plan(name, 512, 192):
            p = "layer%d.%d" % (li, idx)
            y = resnet_ref.basic_block(sd, p, y, stride, ds, True, q=q) if kind == "basic" else q(alternet_ref.attn_block(sd, p, y, hd, ws, shift, True, keep=next(rows)))
        y = q(F.relu(resnet_ref._bn(sd, "bn2", y, True)))
        if dropout_mask is not None:
            y = y * dropout_mask
        y = F.adaptive_avg_pool2d(y, (6, 6)).reshape(y.shape[0], -1)
        y = resnet_ref._bn(sd, "bn3", F.linear(y, q(sd["fc.weight"]), sd["fc.bias"]), True)
    return float(np.linalg.norm(y.numpy() - g["out"]) / np.linalg.norm(g["out"]))


@contextlib.contextmanager
def inject_draws(keeps, dropout_mask):
    """Run the PRODUCT's training forward on injected draws instead of its own: every attention block of nets.AlterNet_SwinV2_FAN gets
    its row of `keeps` (through the module-level attn_block_forward, keep=) and frhip.ops.dropout_mask returns `dropout_mask` (NCHW, the
    reference's layout) permuted to the product's NHWC.  On exit it asserts that every row and the mask were CONSUMED by the code path
    under test: the block ran in training mode with its stochastic depth on and saved exactly the injected row for backward, the tail
    asked for a mask of the injected shape with the keep probability the mask was drawn for.  A run that skips the injection fails."""
    import nets.AlterNet_SwinV2_FAN as A
    from frhip import ops
    orig_block, orig_mask = A.attn_block_forward, ops.dropout_mask
    rows = None if keeps is None else [r.cuda() for r in keeps]
    used = dict(blocks=0, mask=0)

    def block(blk, x, dt, training, save, *a, **kw):
        assert rows is not None and training and blk.drop_path_rate > 0 and used["blocks"] < len(rows)
        assert abs(float(keeps.max()) * (1.0 - blk.drop_path_rate) - 1.0) < 1e-6          # the factors were drawn for this block's rate
        kw["keep"] = rows[used["blocks"]]
        out, s = orig_block(blk, x, dt, training, save, *a, **kw)
        assert s is None or s.keep is kw["keep"]
        used["blocks"] += 1
        return out, s

    def mask(shape, dtype, keep, device, seed=None):
        b, h, w, c = shape
        assert tuple(dropout_mask.shape) == (b, c, h, w) and abs(float(dropout_mask.max()) * keep - 1.0) < 1e-6
        used["mask"] += 1
        return dropout_mask.permute(0, 2, 3, 1).contiguous().to(device=device, dtype=dtype)

    A.attn_block_forward, ops.dropout_mask = block, mask
    try:
        yield used
    finally:
        A.attn_block_forward, ops.dropout_mask = orig_block, orig_mask
    assert used["blocks"] == (0 if keeps is None else len(rows)) and used["mask"] == 1, used


def whole_net_train_on_gpu(net, g, h=112, w=112, keeps=None, dropout_mask=None):
    """one training-mode forward/backward of a product backbone on the fixture's inputs -> (grads by name, embeddings, buffers), CPU.
    keeps / dropout_mask None: the RNG-free pass; else the network as it ships (Dropout 0.5, stochastic depth 0.1) on injected draws."""
    net.train()
    stochastic = keeps is not None or dropout_mask is not None
    if not stochastic:
        net.dropout.p = 0.0                  # the fixtures' RNG-free training pass (Dropout p = 0, stochastic depth off)
        for m in net.modules():
            if hasattr(m, "drop_path_rate"):
                m.drop_path_rate = 0.0
    seed, batch = int(g["seed"]), int(g["batch"])
    with (inject_draws(keeps, dropout_mask) if stochastic else contextlib.nullcontext()):
        y = net(recipe.images(seed + 1, batch, h, w).cuda())
        y.backward(recipe.normal(seed + 2, tuple(y.shape), 0.05).cuda())
        torch.cuda.synchronize()
    return ({k: p.grad.float().cpu() for k, p in net.named_parameters()}, y.detach().float().cpu().numpy(),
            {k: b.detach().cpu() for k, b in net.named_buffers()})
