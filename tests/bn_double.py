"""Float64 restatement of the BatchNorm statistic chain behind csrc/bn.hip, from the column sums on.  TEST-ONLY.

The kernels never see a tensor at this point, only two sums per channel, so neither does this file:

  forward   s1 = sum x, s2 = sum x^2 over `count` values per channel
            mean = s1 / count;  var = max(s2 / count - mean^2, 0)          (biased, clamped as the kernel clamps it)
            invstd = 1 / sqrt(var + eps);  scale = gamma invstd;  shift = beta - mean scale
            running_mean <- (1 - momentum) running_mean + momentum mean
            running_var  <- (1 - momentum) running_var  + momentum var count / (count - 1)     (var itself at count == 1)
  eval      mean = running_mean, invstd = 1 / sqrt(running_var + eps), scale / shift as above
  backward  s1 = sum d, s2 = sum d xhat with d the (masked) upstream gradient and xhat = (y - mean) invstd
            dbeta = s1, dgamma = s2, and  dy = ca d + cb y + cc  with
            training: ca = gamma invstd, cb = -ca invstd s2 / count, cc = ca (mean invstd s2 / count - s1 / count)
            eval:     ca = gamma invstd, cb = cc = 0

Every argument is converted to float64 first and no argument is changed.  eps and momentum are used as given: a caller that compares with
an fp32 kernel passes the fp32 values of its constants (float(numpy.float32(1e-5)))."""
import torch


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


def forward(s1, s2, count, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """-> dict(mean, var, invstd, scale, shift, running_mean, running_var); the running entries are None when none were given"""
    s1, s2, gamma, beta = _d(s1), _d(s2), _d(gamma), _d(beta)
    count = float(count)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=beta - mean * scale, running_mean=None, running_var=None)
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1.0 else var
        out["running_mean"] = (1.0 - momentum) * _d(running_mean) + momentum * mean
        out["running_var"] = (1.0 - momentum) * _d(running_var) + momentum * unbiased
    return out


def eval_state(gamma, beta, running_mean, running_var, eps=1e-5):
    """the state an eval-mode BatchNorm normalises with -> dict(mean, invstd, scale, shift)"""
    gamma, beta, rm, rv = _d(gamma), _d(beta), _d(running_mean), _d(running_var)
    invstd = 1.0 / torch.sqrt(rv + eps)
    scale = gamma * invstd
    return dict(mean=rm.clone(), invstd=invstd, scale=scale, shift=beta - rm * scale)


def backward(s1, s2, count, gamma, mean, invstd, eval_mode=False):
    """-> dict(dgamma, dbeta, ca, cb, cc) from s1 = sum d and s2 = sum d xhat"""
    s1, s2, gamma, mean, invstd = _d(s1), _d(s2), _d(gamma), _d(mean), _d(invstd)
    count = float(count)
    ca = gamma * invstd
    if eval_mode:
        cb, cc = torch.zeros_like(ca), torch.zeros_like(ca)
    else:
        m1, m2 = s1 / count, s2 / count
        cb = -ca * invstd * m2
        cc = ca * (mean * invstd * m2 - m1)
    return dict(dgamma=s2.clone(), dbeta=s1.clone(), ca=ca, cb=cb, cc=cc)


def backward_sums(dout, y, mean, invstd, scale=None, shift=None):
    """the two sums of the backward reduction over a [rows, C] pair: d = dout (y scale + shift > 0) when a mask is given
    -> (d, s1, s2)"""
    dout, y, mean, invstd = _d(dout), _d(y), _d(mean), _d(invstd)
    d = dout if scale is None else dout * ((y * _d(scale) + _d(shift)) > 0)
    return d, d.sum(0), (d * (y - mean) * invstd).sum(0)


def input_grad(d, y, coef):
    """dy = ca d + cb y + cc"""
    return coef["ca"] * _d(d) + coef["cb"] * _d(y) + coef["cc"]
