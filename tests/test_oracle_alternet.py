"""Pin oracle/alternet_ref.py to vectors produced by the real reference nets/AlterNet_SwinV2_FAN.py."""
import numpy as np
import pytest
import torch

from oracle import alternet_ref, recipe, resnet_ref

NOISE = ("proj.bias", "v_bias")


@pytest.mark.parametrize("tag", ["c128_w6", "c512_w3"])
def test_attention_pair(golden, tag):
    g = golden("alternet_pair_" + tag)
    c, heads, ws, res = int(g["c"]), int(g["heads"]), int(g["ws"]), int(g["res"])
    x = recipe.normal(7101, (2, c, res, res)).requires_grad_(True)
    sds, y = [], x
    for j, shift in enumerate((0, ws // 2)):
        spec = alternet_ref.attn_block_spec("blk", c, heads, ws, shift, res)
        sd = alternet_ref.fill_special(recipe.fill_state(spec, 7000 + 10 * heads + j), spec)
        names = [k for k, _, kind in spec if kind in ("linear_w", "linear_b", "bn_w", "bn_b", "logit_scale")]
        for k in names:
            sd[k] = sd[k].clone().requires_grad_(True)
        y = alternet_ref.attn_block(sd, "blk", y, heads, ws, shift, True)
        sds.append((sd, names))
    y.backward(recipe.normal(7102, (2, c, res, res)))
    np.testing.assert_allclose(y.detach().numpy(), g["out"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(x.grad.numpy(), g["dx"], rtol=1e-3, atol=1e-5)
    for j, (sd, names) in enumerate(sds):
        for k in names:
            want = g["b%d.grad.%s" % (j, k[4:])]
            got = sd[k].grad
            got = recipe.summary(got) if (want.shape == (10,) and got.numel() != 10) else got.numpy()
            np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-4 if k.endswith(NOISE) else 2e-5, err_msg=k)


def test_alternet50_eval(golden):
    g = golden("alternet50_b2_eval")
    spec = alternet_ref.alter_spec("AlterNet50")
    assert len(spec) == int(g["n_keys"])
    sd = alternet_ref.fill_special(recipe.fill_state(spec, 7300), spec)
    with torch.no_grad():
        y = alternet_ref.alter_forward(sd, recipe.images(7301, 2, 192, 192), "AlterNet50", False)
    np.testing.assert_allclose(y.numpy(), g["out"], rtol=1e-3, atol=1e-4)


TRAINABLE = ("conv", "linear_w", "linear_b", "bn_w", "bn_b", "logit_scale")


def _whole_net(g, keeps=None, dropout_mask=None):
    """one training-mode forward/backward of the oracle on the fixture's inputs -> the arguments of check_whole_net_train"""
    spec = alternet_ref.alter_spec("AlterNet50")
    sd = alternet_ref.fill_special(recipe.fill_state(spec, int(g["seed"])), spec)
    names = [k for k, _, kind in spec if kind in TRAINABLE]
    for k in names:
        sd[k].requires_grad_(True)
    y = alternet_ref.alter_forward(sd, recipe.images(int(g["seed"]) + 1, int(g["batch"]), 192, 192), "AlterNet50", True,
                                   keeps=keeps, dropout_mask=dropout_mask)
    y.backward(recipe.normal(int(g["seed"]) + 2, tuple(y.shape), 0.05))
    assert {"gprobe." + k for k in names} == {k for k in g if k.startswith("gprobe.")}
    return {k: sd[k].grad for k in names}, y.detach().numpy(), {k: v.detach() for k, v in sd.items()}


def test_alternet50_whole_net_training_mode(golden):
    """/root/reference/nets/AlterNet_SwinV2_FAN.py:637-751 in training mode at 192 x 192, batch 8: stride-2 stem, conv <-> (W-MSA, SW-MSA)
    interleave, bn2 -> ReLU -> Dropout(p = 0 here) -> AAP(6,6) -> fc -> bn3 tail"""
    from wholenet import check_whole_net_train
    g = golden("alternet50_b8_train")
    check_whole_net_train(g, *_whole_net(g), noise=("fc.bias",))


def test_alternet50_whole_net_training_mode_stochastic(golden):
    """the same pass with both random paths ON as the reference trains them: x + drop_path(norm2(attn(x))) with DropPath(0.1) in all
    twelve attention blocks (:334, :372, :444) and Dropout(0.5) between the tail's ReLU and its pool (:667, :745).  The reference ran on
    draws injected from oracle.recipe (tools/make_golden.py: the DropPath stub's second mode, InjectedDropout); the fixture stores the
    two seeds, and stochastic_draws asserts that the regenerated factors still drop what the wiring needs dropped."""
    from wholenet import check_whole_net_train, stochastic_draws
    g = golden("alternet50_b8_train_stochastic")
    keeps, mask = stochastic_draws(g)
    check_whole_net_train(g, *_whole_net(g, keeps, mask), noise=("fc.bias",))


@pytest.mark.parametrize("defect", ["depth_ignored", "rows_shifted", "mask_nhwc_on_nchw"])
def test_stochastic_fixture_rejects_a_defective_whole_net(golden, defect):
    """NEGATIVE CONTROLS: what the stochastic fixture is for.  The oracle with a plausible wiring defect built in must FAIL
    check_whole_net_train at the tolerances the parity tests use:
      depth_ignored      every factor 1 (stochastic depth never applied)
      rows_shifted       block i scales by block i-1's row
      mask_nhwc_on_nchw  the dropout mask's memory read in the other layout: an NHWC-ordered mask multiplied onto the NCHW tensor
    (the remaining defects run at block size: test_stochastic_check_rejects_a_defective_block_pair)."""
    from wholenet import check_whole_net_train, stochastic_draws
    g = golden("alternet50_b8_train_stochastic")
    keeps, mask = stochastic_draws(g)
    b, c, h, w = mask.shape
    if defect == "depth_ignored":
        keeps = None
    elif defect == "rows_shifted":
        keeps = torch.roll(keeps, 1, 0)
    else:
        mask = mask.permute(0, 2, 3, 1).contiguous().view(b, c, h, w)
    with pytest.raises(AssertionError):
        check_whole_net_train(g, *_whole_net(g, keeps, mask), noise=("fc.bias",))


def _pair_net(keeps, mask, block=alternet_ref.attn_block, c=128, heads=4, ws=6, res=12, emd=64, batch=8):
    """a (W-MSA, SW-MSA) pair of the alternet_pair_c128_w6 size under stochastic depth + the AlterNet tail (bn2 -> ReLU -> dropout ->
    AAP(6,6) -> fc -> bn3), forward/backward -> the arguments of check_whole_net_train"""
    spec = []
    for j, shift in enumerate((0, ws // 2)):
        spec += alternet_ref.attn_block_spec("layer1.%d" % j, c, heads, ws, shift, res)
    spec += (resnet_ref._bn_spec("bn2", c) + [("fc.weight", (emd, c * 36), "linear_w"), ("fc.bias", (emd,), "linear_b")] +
             resnet_ref._bn_spec("bn3", emd))
    sd = alternet_ref.fill_special(recipe.fill_state(spec, 7600), spec)
    names = [k for k, _, kind in spec if kind in TRAINABLE]
    for k in names:
        sd[k].requires_grad_(True)
    y = recipe.normal(7601, (batch, c, res, res))
    for j, shift in enumerate((0, ws // 2)):
        y = block(sd, "layer1.%d" % j, y, heads, ws, shift, True, keep=keeps[j])
    y = alternet_ref.tail(sd, y, True, mask)
    y.backward(recipe.normal(7602, tuple(y.shape), 0.05))
    return names, ({k: sd[k].grad for k in names}, y.detach().numpy(), {k: v.detach() for k, v in sd.items()})


def _forward_only_block(sd, p, x, heads, ws, shift, training, keep=None):
    """defect: the factor honoured in forward, forgotten in backward"""
    n = alternet_ref.attn_block(sd, p, x, heads, ws, shift, training) - x
    return x + (n * keep.view(-1, 1, 1, 1)).detach() + (n - n.detach())


@pytest.mark.parametrize("defect", [None, "factors_unscaled", "forward_only", "mask_nchw_as_nhwc"])
def test_stochastic_check_rejects_a_defective_block_pair(defect):
    """NEGATIVE CONTROLS at the alternet_pair_c128_w6 block size (the whole net would cost 5 s of CPU apiece): the correct oracle is the
    yardstick here, held in the format of a whole-net fixture, and check_whole_net_train must reject
      factors_unscaled   {0, 1} instead of {0, 1/keep}: the missing 1/keep
      forward_only       x + (n f).detach() + (n - n.detach()): a backward consumer that forgot the factor
      mask_nchw_as_nhwc  the converse of the whole-net layout defect: the NCHW mask's memory taken for an NHWC one
    and accept the unmodified oracle (None: the control of the controls)."""
    from wholenet import check_whole_net_train
    keeps = recipe.keep_factors(7424, 12, 8, 0.9)[:2]
    assert (keeps[0] == 0).sum() == 2 and (keeps[1] == 0).sum() == 2 and not ((keeps[0] == 0) & (keeps[1] == 0)).any()
    mask = recipe.dropout_mask(7603, (8, 128, 12, 12), 0.5)
    names, (grads, out, sd) = _pair_net(keeps, mask)
    g = {"out": out, "gprobe16k.fc.weight": recipe.probe(grads["fc.weight"], 16384)}
    g.update({"gprobe." + k: recipe.probe(grads[k]) for k in names})
    g.update({"after." + k: recipe.probe(v.float()) for k, v in sd.items() if "running" in k})
    noise = ("fc.bias",)
    if defect is None:
        check_whole_net_train(g, *_pair_net(keeps, mask)[1], noise=noise)
        return
    if defect == "factors_unscaled":
        bad = _pair_net((keeps != 0).float(), mask)
    elif defect == "forward_only":
        bad = _pair_net(keeps, mask, block=_forward_only_block)
    else:
        bad = _pair_net(keeps, mask.contiguous().view(8, 12, 12, 128).permute(0, 3, 1, 2))
    with pytest.raises(AssertionError):
        check_whole_net_train(g, *bad[1], noise=noise)
    if defect == "forward_only":          # the defect is in backward ALONE: same embeddings, and still rejected
        np.testing.assert_allclose(bad[1][1], out, rtol=1e-5, atol=1e-6)


def _recipe_two_steps(g):
    from oracle import train_ref
    from wholenet import stochastic_draws
    stochastic = "keep_seed" in g
    C, B, steps, rate, lr = int(g["C"]), int(g["B"]), int(g["steps"]), float(g["rate"]), float(g["lr"])
    spec = alternet_ref.alter_spec("AlterNet50")
    sd = alternet_ref.fill_special(recipe.fill_state(spec, int(g["seed"])), spec)
    names = [k for k, _, kind in spec if kind in TRAINABLE]
    W = recipe.normal(9101, (C, 512), 0.01)
    opt = train_ref.AdamWState(lr, tuple(g["betas"]), float(g["eps"]), float(g["wd"]))
    for st in range(steps):
        keeps, mask = stochastic_draws(g, st) if stochastic else (None, None)                  # fresh draws every step
        fwd = lambda work, img: alternet_ref.alter_forward(work, img, "AlterNet50", True, keeps=keeps, dropout_mask=mask)      # noqa: E731
        img, ids = recipe.images(9110 + 10 * st, B, 192, 192), recipe.labels(9111 + 10 * st, B, C)
        torch.manual_seed(9200 + st)
        u = [torch.rand(C)]
        out = train_ref.train_step(sd, W, img, ids, None, C, opt, sample_rate=rate, uniforms=u, forward=fwd, names=names)
        np.testing.assert_allclose(out["loss"].item(), g["losses"][st], rtol=1e-3 if st == 0 else 1e-2)
        np.testing.assert_allclose(out["grad_norm"].item(), g["grad_norms"][st], rtol=5e-3 if st == 0 else 5e-2)
        assert np.array_equal(out["index"].numpy(), g["index_step%d" % st])
        if st == 0:
            for k in [k[6:] for k in g if k.startswith("grad0.")]:
                want = g["grad0." + k]
                np.testing.assert_allclose(recipe.probe(out["grads"][k])[1:], want[1:], rtol=1e-2, atol=5e-2 * want[1] / out["grads"][k].numel() ** 0.5, err_msg=k)
    for k in [k[6:] for k in g if k.startswith("after.") and not k.startswith("after.head")]:
        got, want = recipe.probe(sd[k].float()), g["after." + k]
        np.testing.assert_allclose(got[1], want[1], rtol=2e-3, err_msg=k)
        assert np.abs(got[2:] - want[2:]).max() <= 2.2 * lr * steps, k


def test_shipped_recipe_two_steps(golden):
    """/root/reference/main/train.sh:12 end to end (AlterNet50 @192 + PartialFCAdamW rate 0.3 + AdamW lr 5e-4 + clip 5), two steps on fresh batches"""
    _recipe_two_steps(golden("recipe_alternet50_adamw_rate03"))


def test_shipped_recipe_two_steps_stochastic(golden):
    """the same two steps as the recipe really runs them: DropPath(0.1) and Dropout(0.5) on, fresh injected draws per step (seed + step)"""
    _recipe_two_steps(golden("recipe_alternet50_adamw_rate03_stochastic"))
