"""tests/bn_double.py (the float64 reference the GPU tests of the BatchNorm reductions compare with) against float64 F.batch_norm and
autograd: training and eval mode, with and without the ReLU behind the BatchNorm, to 1e-12."""
import pytest
import torch
import torch.nn.functional as F

import bn_double

TOL = dict(rtol=1e-12, atol=1e-12)
MOMENTUM, EPS = 0.1, 1e-5


def _data(seed, rows, c):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(y=r(rows, c) * 1.5 + 0.3, dout=r(rows, c), gamma=1 + 0.2 * r(c), beta=0.3 * r(c), rm=0.2 * r(c), rv=1 + 0.3 * r(c).abs())


def _autograd(t, training, relu):
    y, gamma, beta = (t[k].clone().requires_grad_(True) for k in ("y", "gamma", "beta"))
    rm, rv = t["rm"].clone(), t["rv"].clone()
    out = F.batch_norm(y, rm, rv, gamma, beta, training, MOMENTUM, EPS)
    (F.relu(out) if relu else out).backward(t["dout"])
    return out.detach(), rm, rv, y.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,c", [(2, 3), (37, 8), (200, 5)])
def test_training_mode(rows, c, relu):
    t = _data(rows, rows, c)
    out, rm, rv, dy, dgamma, dbeta = _autograd(t, True, relu)
    y = t["y"]
    st = bn_double.forward(y.sum(0), (y * y).sum(0), rows, t["gamma"], t["beta"], t["rm"], t["rv"], MOMENTUM, EPS)
    torch.testing.assert_close(st["mean"], y.mean(0), **TOL)
    torch.testing.assert_close(st["invstd"], 1.0 / torch.sqrt(y.var(0, unbiased=False) + EPS), **TOL)
    torch.testing.assert_close(y * st["scale"] + st["shift"], out, **TOL)
    torch.testing.assert_close(st["running_mean"], rm, **TOL)
    torch.testing.assert_close(st["running_var"], rv, **TOL)
    mask = (st["scale"], st["shift"]) if relu else (None, None)
    d, s1, s2 = bn_double.backward_sums(t["dout"], y, st["mean"], st["invstd"], *mask)
    if relu:
        assert torch.equal(d, t["dout"] * (out > 0))
    b = bn_double.backward(s1, s2, rows, t["gamma"], st["mean"], st["invstd"])
    torch.testing.assert_close(b["dgamma"], dgamma, **TOL)
    torch.testing.assert_close(b["dbeta"], dbeta, **TOL)
    torch.testing.assert_close(bn_double.input_grad(d, y, b), dy, **TOL)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,c", [(1, 3), (37, 8)])
def test_eval_mode(rows, c, relu):
    t = _data(100 + rows, rows, c)
    out, rm, rv, dy, dgamma, dbeta = _autograd(t, False, relu)
    assert torch.equal(rm, t["rm"]) and torch.equal(rv, t["rv"])
    y = t["y"]
    st = bn_double.eval_state(t["gamma"], t["beta"], t["rm"], t["rv"], EPS)
    torch.testing.assert_close(y * st["scale"] + st["shift"], out, **TOL)
    mask = (st["scale"], st["shift"]) if relu else (None, None)
    d, s1, s2 = bn_double.backward_sums(t["dout"], y, st["mean"], st["invstd"], *mask)
    b = bn_double.backward(s1, s2, rows, t["gamma"], st["mean"], st["invstd"], eval_mode=True)
    assert not b["cb"].any() and not b["cc"].any()
    torch.testing.assert_close(b["dgamma"], dgamma, **TOL)
    torch.testing.assert_close(b["dbeta"], dbeta, **TOL)
    torch.testing.assert_close(bn_double.input_grad(d, y, b), dy, **TOL)


def test_a_single_value_per_channel_keeps_the_biased_variance():
    """count == 1: F.batch_norm refuses to train on it, the kernels do not; var is 0, the n / (n - 1) correction is skipped"""
    y = torch.tensor([[1.5, -2.0, 0.0]], dtype=torch.float64)
    rm, rv = torch.tensor([0.1, 0.2, 0.3]), torch.tensor([1.0, 2.0, 3.0])
    st = bn_double.forward(y.sum(0), (y * y).sum(0), 1, torch.ones(3), torch.zeros(3), rm, rv, MOMENTUM, EPS)
    assert torch.equal(st["mean"], y[0]) and not st["var"].any()
    torch.testing.assert_close(st["invstd"], torch.full((3,), EPS ** -0.5, dtype=torch.float64), **TOL)
    torch.testing.assert_close(st["running_var"], (1 - MOMENTUM) * rv.double(), **TOL)
    torch.testing.assert_close(st["running_mean"], (1 - MOMENTUM) * rm.double() + MOMENTUM * y[0], **TOL)


def test_negative_variance_is_clamped_and_no_argument_changes():
    s1, s2 = torch.tensor([4.0, 4.0]), torch.tensor([3.0, 5.0])          # count 4: s2 / 4 - 1 = -0.25 and +0.25
    rm, rv = torch.zeros(2), torch.ones(2)
    st = bn_double.forward(s1, s2, 4, torch.ones(2), torch.zeros(2), rm, rv, 1.0, EPS)
    assert st["var"].tolist() == [0.0, 0.25]
    assert st["running_var"].tolist() == [0.0, 0.25 * 4 / 3] and st["running_mean"].tolist() == [1.0, 1.0]
    assert torch.equal(rm, torch.zeros(2)) and torch.equal(rv, torch.ones(2))
    assert bn_double.forward(s1, s2, 4, torch.ones(2), torch.zeros(2))["running_mean"] is None
