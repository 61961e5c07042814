"""Tensor-level wrappers over the C ABI (torch is used for device memory + the current HIP stream only)."""
import math
import weakref

import ctypes

import torch

from . import _abi
from ._abi import DT_BF16, DT_F32, check, lib

_DT = {torch.bfloat16: DT_BF16, torch.float32: DT_F32}


def dt_of(t):
    return _DT[t.dtype]


def epv(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _s():
    # raw hipStream_t of torch's current stream (the public torch.cuda.current_stream() costs ~9 us per call)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "frhip ops need contiguous CUDA tensors"
    return t.data_ptr()


def nt_block_m(k):
    return lib().frhip_nt_block_m(k)


# ------------------------------------------------------------------------------------------ convolution
def conv_out_hw(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def conv_fwd(x, w, stride, pad, want_stats=True):
    """x [N,H,W,C], w [K,R,S,C] (same dtype) -> y [N,Ho,Wo,K], stats partial [tiles,2,K] fp32 or None"""
    n, h, wd, c = x.shape
    k, r, s, c2 = w.shape
    assert c == c2 and x.dtype == w.dtype
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad)
    y = torch.empty((n, ho, wo, k), dtype=x.dtype, device=x.device)
    part = None
    if want_stats:
        rows = lib().frhip_conv_stat_rows(dt_of(x), n * ho * wo, k, h, wd, c, r, s, stride, pad)
        part = torch.empty((rows, 2, k), dtype=torch.float32, device=x.device)
    check(lib().frhip_conv_fwd(dt_of(x), _p(x), _p(w), _p(y), _p(part), n, h, wd, c, k, r, s, stride, pad, _s()),
          "frhip_conv_fwd")
    return y, part


def conv_fwd_affine(x, w, st, stride, pad, relu=False, residual=None):
    """inference: y = [relu](conv(x, w) * st.scale + st.shift + residual) -- eval-mode BatchNorm (bn_eval_affine) folded into the
    convolution's store epilogue; residual shaped like y"""
    n, h, wd, c = x.shape
    k, r, s, c2 = w.shape
    assert c == c2 and x.dtype == w.dtype
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad)
    y = torch.empty((n, ho, wo, k), dtype=x.dtype, device=x.device)
    if residual is not None and (tuple(residual.shape) != tuple(y.shape) or residual.dtype != y.dtype):
        raise ValueError("conv_fwd_affine: residual must have the shape and dtype of the output")
    check(lib().frhip_conv_fwd_affine(dt_of(x), _p(x), _p(w), _p(y), _p(st.scale), _p(st.shift), int(relu), _p(residual),
                                      n, h, wd, c, k, r, s, stride, pad, _s()), "frhip_conv_fwd_affine")
    return y


def conv_dgrad(dy, wt, x_shape, r, s, stride, pad, residual=None, out=None, bnred=None, residual_stride=1):
    """dy [N,Ho,Wo,K], wt [C,R,S,K] -> dx [N,H,W,C] (+ residual).

    residual_stride=2: `residual` is the compact [N,(H+1)/2,(W+1)/2,C] gradient of a stride-2 1x1 shortcut, added on the
    even pixels only.
    bnred=(y_bn, st, relu_mask[, rowscale, rows_per, keep_scale]): dx is the upstream gradient of a BatchNorm with saved input y_bn and
    batch state st; the BN-backward partial sums come out of the epilogue and (dx, partial) is returned -- pass partial to bn_backward.
    With rowscale (fp32 per sample: 0 or keep_scale) the BatchNorm sits under stochastic depth and the sums describe dx * rowscale[sample]."""
    n, h, wd, c = x_shape
    k = dy.shape[3]
    dx = out if out is not None else torch.empty(x_shape, dtype=dy.dtype, device=dy.device)
    if residual is not None:
        want = (n, h, wd, c) if residual_stride == 1 else (n, (h + 1) // 2, (wd + 1) // 2, c)
        if tuple(residual.shape) != want or residual.dtype != dy.dtype:
            raise ValueError("conv_dgrad: residual must be %s %s" % (want, dy.dtype))
    if bnred is None and residual_stride == 1:
        check(lib().frhip_conv_dgrad(dt_of(dy), _p(dy), _p(wt), _p(dx), _p(residual), n, h, wd, c, k, r, s, stride, pad, _s()),
              "frhip_conv_dgrad")
        return dx
    part = y_bn = st = None
    relu_mask = False
    rowscale = None
    if bnred is not None:
        y_bn, st, relu_mask = bnred[:3]
        if len(bnred) > 3 and bnred[3] is not None:
            rowscale, rows_per, keep_scale = bnred[3], int(bnred[4]), float(bnred[5])
            assert rowscale.dtype == torch.float32 and rowscale.is_contiguous() and rowscale.numel() * rows_per == n * h * wd
        if tuple(y_bn.shape) != tuple(x_shape) or y_bn.dtype != dy.dtype:
            raise ValueError("conv_dgrad(bnred): y_bn must have the shape and dtype of dx")
        rows = lib().frhip_dgrad_stat_rows(dt_of(dy), n, h, wd, c, k, r, s, stride, pad)
        part = torch.empty((rows, 2, c), dtype=torch.float32, device=dy.device)
    if rowscale is not None:
        check(lib().frhip_conv_dgrad_fused_rs(dt_of(dy), _p(dy), _p(wt), _p(dx), _p(residual), residual_stride, _p(y_bn), _p(st.mean),
                                              _p(st.invstd), _p(st.scale) if relu_mask else None, _p(st.shift) if relu_mask else None,
                                              _p(rowscale), rows_per, keep_scale, _p(part), n, h, wd, c, k, r, s, stride, pad, _s()),
              "frhip_conv_dgrad_fused_rs")
        return dx, part
    check(lib().frhip_conv_dgrad_fused(dt_of(dy), _p(dy), _p(wt), _p(dx), _p(residual), residual_stride, _p(y_bn),
                                       _p(st.mean) if st else None, _p(st.invstd) if st else None,
                                       _p(st.scale) if relu_mask else None, _p(st.shift) if relu_mask else None, _p(part),
                                       n, h, wd, c, k, r, s, stride, pad, _s()), "frhip_conv_dgrad_fused")
    return dx if bnred is None else (dx, part)


_FUSABLE = {}


def conv_bnrelu_fusable(x, w, stride, pad):
    """can conv(relu(bn(x)), w) run with the BatchNorm-apply + ReLU folded into the operand path (forward AND weight gradient)?"""
    n, h, wd, c = x.shape
    k, r, s, _ = w.shape
    key = (x.dtype, n, h, wd, c, k, r, s, stride, pad)
    hit = _FUSABLE.get(key)
    if hit is None:
        hit = _FUSABLE[key] = x.dtype in _DT and \
            bool(lib().frhip_conv_bnrelu_fusable(dt_of(x), h, wd, c, k, r, s, stride, pad)) and \
            bool(lib().frhip_conv_wgrad_bnrelu_fusable(dt_of(x), n, h, wd, c, k, r, s, stride, pad))
    return hit


def conv_fwd_bnrelu(x, st, w, stride, pad, want_stats=True, act_out=None):
    """y = conv(relu(x * st.scale + st.shift), w) without a separate BatchNorm-apply pass (x = the BatchNorm's input); act_out (like
    x, optional) receives the activated tensor on the way"""
    n, h, wd, c = x.shape
    k, r, s, c2 = w.shape
    assert c == c2 and x.dtype == w.dtype
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad)
    y = torch.empty((n, ho, wo, k), dtype=x.dtype, device=x.device)
    part = None
    if want_stats:
        rows = lib().frhip_conv_stat_rows(dt_of(x), n * ho * wo, k, h, wd, c, r, s, stride, pad)
        part = torch.empty((rows, 2, k), dtype=torch.float32, device=x.device)
    check(lib().frhip_conv_fwd_bnrelu(dt_of(x), _p(x), _p(st.scale), _p(st.shift), _p(w), _p(y), _p(part), _p(act_out), n, h, wd, c, k,
                                      r, s, stride, pad, _s()), "frhip_conv_fwd_bnrelu")
    return y, part


_WORKSPACES = {}
WORKSPACE_BYTES = 160 << 20


def workspace(device):
    """one 160 MB split-K scratch per (device, stream): kernels on different streams never share it"""
    key = (torch.device(device).index, _s())
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = torch.empty(WORKSPACE_BYTES // 4, dtype=torch.float32, device=device)
    return ws


def conv_wgrad(dy, x, dw, r, s, stride, pad, splits=0):
    """dw [K,R,S,C] fp32 (zeroed by caller) += wgrad(dy [N,Ho,Wo,K], x [N,H,W,C])"""
    n, h, wd, c = x.shape
    k = dy.shape[3]
    ws = workspace(x.device)
    check(lib().frhip_conv_wgrad(dt_of(x), _p(dy), _p(x), _p(dw), n, h, wd, c, k, r, s, stride, pad, splits,
                                 _p(ws), ws.numel() * 4, _s()), "frhip_conv_wgrad")
    return dw


WGRAD_FAMILIES = ("tap128", "tap256", "taps9", "rows")


def wgrad_plan(dtype, n, h, w, c, kc, ldp, r, s, stride, pad, splits=0, workspace_bytes=WORKSPACE_BYTES, overwrite=False, transform=False):
    """(family, instantiation, splits, ksteps, ksteps_per_split, store, reduce groups, slabs per group) of the weight-gradient launch with
    these arguments (frhip_wgrad_plan; workspace_bytes None = no workspace).  Touches no device."""
    plan = (ctypes.c_int * 8)()
    check(lib().frhip_wgrad_plan(dtype, n, h, w, c, kc, ldp, r, s, stride, pad, splits, workspace_bytes is not None, workspace_bytes or 0,
                                 int(overwrite), int(transform), plan), "frhip_wgrad_plan")
    return tuple(plan)


CHAIN_SLAB_BYTES = 128 << 20
_CHAIN_SLABS = {}


def chain_slabs(device):
    """two K-split slab buffers per (device, stream) for chained weight gradients: launch i writes one while it sums the other"""
    key = (torch.device(device).index, _s())
    bufs = _CHAIN_SLABS.get(key)
    if bufs is None:
        bufs = _CHAIN_SLABS[key] = [torch.empty(CHAIN_SLAB_BYTES // 4, dtype=torch.float32, device=device) for _ in range(2)]
    return bufs


def conv_wgrad_chain_ok(dy, x, r, s, stride, pad):
    n, h, wd, c = x.shape
    return x.dtype == torch.bfloat16 and bool(lib().frhip_conv_wgrad_chain_ok(dt_of(x), n, h, wd, c, dy.shape[3], r, s, stride, pad))


def conv_wgrad_chain(dy, x, dw, slabs, prev=None):
    """3x3 / stride-1 weight gradient on 14 x 14 maps as one link of a chain (frhip_conv_wgrad_chain): its K-split slabs go to
    `slabs`, the slabs of the previous link `prev` are added to THAT link's dw in this launch's prologue.  Returns this link's
    descriptor (dw, slabs, k, c, splits): hand it to the next link or to conv_wgrad_chain_finish."""
    n, h, wd, c = x.shape
    k = dy.shape[3]
    sp = ctypes.c_int(0)
    pdw, pslabs, pk, pc, psp = prev if prev is not None else (None, None, 0, 0, 0)
    check(lib().frhip_conv_wgrad_chain(dt_of(x), _p(dy), _p(x), n, h, wd, c, k, _p(slabs), slabs.numel() * 4, _p(pdw), _p(pslabs), pk, pc, psp,
                                       ctypes.byref(sp), _s()), "frhip_conv_wgrad_chain")
    return (dw, slabs, k, c, sp.value)


def conv_wgrad_chain_finish(link):
    dw, slabs, k, c, sp = link
    check(lib().frhip_conv_wgrad_chain_finish(_p(dw), _p(slabs), k, c, sp, _s()), "frhip_conv_wgrad_chain_finish")


def conv_wgrad_bnrelu(dy, x, st, dw, r, s, stride, pad, splits=0):
    """dw += wgrad(dy, relu(x * st.scale + st.shift)): x is the saved BatchNorm input, the activation is re-formed in LDS"""
    n, h, wd, c = x.shape
    k = dy.shape[3]
    ws = workspace(x.device)
    check(lib().frhip_conv_wgrad_bnrelu(dt_of(x), _p(dy), _p(x), _p(st.scale), _p(st.shift), _p(dw), n, h, wd, c, k, r, s, stride, pad,
                                        splits, _p(ws), ws.numel() * 4, _s()), "frhip_conv_wgrad_bnrelu")
    return dw


def gemm_nt(a, b, out=None, splits=1, atomic_f32=False):
    m, k = a.shape
    n = b.shape[0]
    if out is None:
        out = (torch.zeros((m, n), dtype=torch.float32, device=a.device) if atomic_f32
               else torch.empty((m, n), dtype=a.dtype, device=a.device))
    check(lib().frhip_gemm_nt(dt_of(a), _p(a), _p(b), _p(out), m, n, k, splits, int(atomic_f32), _s()), "frhip_gemm_nt")
    return out


def gemm_nt_splitk(a, b, bias=None, splits=16):
    """fp32 out[m][n] = a [m,k] @ b [n,k]^T + bias, K split with per-split slabs added in a fixed order (deterministic)"""
    m, k = a.shape
    n = b.shape[0]
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    ws = workspace(a.device)
    check(lib().frhip_gemm_nt_splitk(dt_of(a), _p(a), _p(b), _p(bias), _p(out), m, n, k, splits, _p(ws), ws.numel() * 4, _s()),
          "frhip_gemm_nt_splitk")
    return out


def linear_fwd(a, w, bias=None, want_act=False, want_stats=False):
    """nn.Linear with its epilogue: out = a [M,K] @ w [N,K]^T + bias (fp32 [N]); act = gelu(out) when want_act;
    part = BatchNorm partial sums of out when want_stats.  Returns (out, act, part)."""
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k and a.dtype == w.dtype
    out = torch.empty((m, n), dtype=a.dtype, device=a.device)
    act = torch.empty_like(out) if want_act else None
    part = None
    if want_stats:
        rows = lib().frhip_conv_stat_rows(dt_of(a), m, n, 1, 1, k, 1, 1, 1, 0)
        part = torch.empty((rows, 2, n), dtype=torch.float32, device=a.device)
    check(lib().frhip_linear_fwd(dt_of(a), _p(a), _p(w), _p(bias), _p(out), _p(act), _p(part), m, n, k, _s()), "frhip_linear_fwd")
    return out, act, part


def linear_dgrad_gelu(dy, wt, pre, want_colsum=True, colsum_into=None):
    """dx = (dy [M,K] @ wt [N,K]^T) * gelu'(pre [M,N]); colsum [N] fp32 = sum over rows of dx (the bias gradient).
    colsum_into (fp32 [N]): the column sums are ADDED into it by one launch (frhip_sum_partials) and it is returned"""
    m, k = dy.shape
    n = wt.shape[0]
    assert tuple(pre.shape) == (m, n) and pre.dtype == dy.dtype == wt.dtype
    dx = torch.empty((m, n), dtype=dy.dtype, device=dy.device)
    part = None
    if want_colsum:
        rows = lib().frhip_conv_stat_rows(dt_of(dy), m, n, 1, 1, k, 1, 1, 1, 0)
        part = torch.empty((rows, 2, n), dtype=torch.float32, device=dy.device)
    check(lib().frhip_linear_dgrad_gelu(dt_of(dy), _p(dy), _p(wt), _p(pre), _p(dx), _p(part), m, n, k, _s()),
          "frhip_linear_dgrad_gelu")
    if want_colsum and colsum_into is not None:
        check(lib().frhip_sum_partials(_p(part), part.shape[0], n, 0, _p(colsum_into), _s()), "frhip_sum_partials")
        return dx, colsum_into
    return dx, (part[:, 0].sum(0) if want_colsum else None)


def gemm_tn(p, q, out, kc=None, splits=0, overwrite=False):
    """out[kc][c] fp32 += sum_m p[m][:kc] * q[m][:c]      (overwrite: out = ..., out need not be initialised)"""
    m, ldp = p.shape
    c = q.shape[1]
    kc = ldp if kc is None else kc
    ws = workspace(p.device)
    if overwrite:
        check(lib().frhip_gemm_tn_overwrite(dt_of(p), _p(p), _p(q), _p(out), m, kc, ldp, c, _p(ws), ws.numel() * 4, _s()),
              "frhip_gemm_tn_overwrite")
        return out
    check(lib().frhip_gemm_tn(dt_of(p), _p(p), _p(q), _p(out), m, kc, ldp, c, splits, _p(ws), ws.numel() * 4, _s()),
          "frhip_gemm_tn")
    return out


# ------------------------------------------------------------------------------------------ batch norm
def _colreduce_blocks(rows, c, dtype_code):
    nb = lib().frhip_colreduce_blocks(rows, c, dtype_code)
    if nb <= 0:
        raise _abi.FrhipError("frhip: the element-wise kernels do not serve %d channels in this dtype" % c)
    return nb


def colstats(x2d):
    rows, c = x2d.shape
    nb = _colreduce_blocks(rows, c, dt_of(x2d))
    part = torch.empty((nb, 2, c), dtype=torch.float32, device=x2d.device)
    check(lib().frhip_colstats(dt_of(x2d), _p(x2d), rows, c, _p(part), _s()), "frhip_colstats")
    return part


class BNState:
    """Per-layer fp32 vectors produced by the forward finalize and consumed by apply / backward.
    eval: normalised with the running statistics (bn_eval_state): its backward is dy = gamma * invstd * d (frhip_bn_bwd_finalize_eval)."""
    __slots__ = ("mean", "invstd", "scale", "shift", "count", "eval")

    def __init__(self):
        self.eval = False


def _bwd_finalize(part, scratch, c, count, gamma, st, dgamma, dbeta, coef):
    """(ca, cb, cc) into coef [3, c] and dgamma / dbeta (None: not accumulated) from the BatchNorm-backward partial sums"""
    fn = lib().frhip_bn_bwd_finalize_eval if st.eval else lib().frhip_bn_bwd_finalize
    check(fn(_p(part), part.shape[0], _p(scratch), c, float(count), _p(gamma), _p(st.mean), _p(st.invstd), _p(dgamma), _p(dbeta),
             _p(coef[0]), _p(coef[1]), _p(coef[2]), _s()), "frhip_bn_bwd_finalize_eval" if st.eval else "frhip_bn_bwd_finalize")


def _bn_state(c, device, count, affine_only=False):
    """BNState whose vectors are rows of one fresh fp32 buffer; affine_only: scale and shift alone (mean = invstd = None)"""
    st = BNState()
    buf = torch.empty((2 if affine_only else 4, c), dtype=torch.float32, device=device)
    st.mean, st.invstd, st.scale, st.shift = (None, None, buf[0], buf[1]) if affine_only else (buf[0], buf[1], buf[2], buf[3])
    st.count = count
    return st


def bn_standin_state(gamma, beta, k, count):
    """BNState(mean = beta, invstd = gamma / (gamma^2 + (k beta)^2 + 1e-20), scale = 1, shift = 0): frhip_bn_standin_state, one launch"""
    c = gamma.numel()
    st = _bn_state(c, gamma.device, count)
    check(lib().frhip_bn_standin_state(c, _p(gamma), _p(beta), float(k), _p(st.mean), _p(st.invstd), _p(st.scale), _p(st.shift), _s()),
          "frhip_bn_standin_state")
    return st


def bn_finalize(part, count, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, scratch=None):
    c = gamma.numel()
    dev = gamma.device
    st = _bn_state(c, dev, float(count))
    if scratch is None:
        scratch = torch.empty((64 * 2 * c,), dtype=torch.float32, device=dev)
    check(lib().frhip_bn_finalize(_p(part), part.shape[0], _p(scratch), c, float(count), _p(gamma), _p(beta),
                                  _p(running_mean), _p(running_var), momentum, eps, _p(st.mean), _p(st.invstd),
                                  _p(st.scale), _p(st.shift), _s()), "frhip_bn_finalize")
    return st


def bn_eval_affine(gamma, beta, running_mean, running_var, eps=1e-5):
    c = gamma.numel()
    st = _bn_state(c, gamma.device, 0.0, affine_only=True)
    check(lib().frhip_bn_eval_affine(c, _p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, _p(st.scale),
                                     _p(st.shift), _s()), "frhip_bn_eval_affine")
    return st


def bn_eval_state(gamma, beta, running_mean, running_var, eps=1e-5):
    """eval-mode BatchNorm state of a pass that is differentiated: bn_eval_affine's scale / shift plus mean = running_mean and
    invstd = rsqrt(running_var + eps) (frhip_bn_eval_state, one launch)"""
    c = gamma.numel()
    st = _bn_state(c, gamma.device, 0.0)
    st.eval = True
    check(lib().frhip_bn_eval_state(c, _p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, _p(st.mean), _p(st.invstd),
                                    _p(st.scale), _p(st.shift), _s()), "frhip_bn_eval_state")
    return st


def bn_apply(y, st, relu=False, res=None, res_st=None, out=None, rowscale=None, rows_per=0):
    """rowscale [groups] fp32 + rows_per: out = res + rowscale[row // rows_per] * (y * scale + shift) (stochastic depth)"""
    c = y.shape[-1]
    rows = y.numel() // c
    out = torch.empty_like(y) if out is None else out
    if rowscale is not None:
        assert not relu and res_st is None and rowscale.dtype == torch.float32 and rows == rowscale.numel() * rows_per
        check(lib().frhip_bn_apply_rs(dt_of(y), _p(y), _p(st.scale), _p(st.shift), _p(res), _p(rowscale), rows_per, _p(out), rows, c,
                                      _s()), "frhip_bn_apply_rs")
        return out
    check(lib().frhip_bn_apply(dt_of(y), _p(y), _p(st.scale), _p(st.shift), _p(res),
                               _p(res_st.scale) if res_st is not None else None,
                               _p(res_st.shift) if res_st is not None else None,
                               int(relu), _p(out), rows, c, _s()), "frhip_bn_apply")
    return out


def bn_backward(dout, y, st, gamma, dgamma, dbeta, relu_mask=False, out=None, scratch=None, part=None, rowscale=None, rows_per=0):
    """dy of BN (optionally through the ReLU that follows it); accumulates dgamma/dbeta (fp32, caller-zeroed; None: not wanted).
    An eval-mode state (bn_eval_state) takes the eval-mode finalize: dy = gamma * invstd * d.
    part: BN-backward partial sums already produced by conv_dgrad(bnred=...) for this (dout, y) pair.
    rowscale / rows_per: the BatchNorm's output was scaled per sample in the forward pass (bn_apply(rowscale=...)): dout is scaled
    likewise inside the reduction and the apply pass"""
    c = y.shape[-1]
    rows = y.numel() // c
    dev = y.device
    rs = rowscale is not None
    if rs:
        assert not relu_mask and rowscale.dtype == torch.float32 and rows == rowscale.numel() * rows_per
    ms = _p(st.scale) if relu_mask else None
    mb = _p(st.shift) if relu_mask else None
    if part is None:               # else: the kernel that produced dout already took the sums (conv_dgrad(bnred=...))
        nb = _colreduce_blocks(rows, c, dt_of(y))
        part = torch.empty((nb, 2, c), dtype=torch.float32, device=dev)
        if rs:
            check(lib().frhip_bn_bwd_reduce_rs(dt_of(y), _p(dout), _p(y), _p(st.mean), _p(st.invstd), _p(rowscale), rows_per, rows, c,
                                               _p(part), _s()), "frhip_bn_bwd_reduce_rs")
        else:
            check(lib().frhip_bn_bwd_reduce(dt_of(y), _p(dout), _p(y), _p(st.mean), _p(st.invstd), ms, mb, rows, c, _p(part), _s()),
                  "frhip_bn_bwd_reduce")
    coef = torch.empty((3, c), dtype=torch.float32, device=dev)
    if scratch is None:
        scratch = torch.empty((64 * 2 * c,), dtype=torch.float32, device=dev)
    _bwd_finalize(part, scratch, c, rows, gamma, st, dgamma, dbeta, coef)
    dy = torch.empty_like(y) if out is None else out
    if rs:
        check(lib().frhip_bn_bwd_apply_rs(dt_of(y), _p(dout), _p(y), _p(coef[0]), _p(coef[1]), _p(coef[2]), _p(rowscale), rows_per,
                                          _p(dy), rows, c, _s()), "frhip_bn_bwd_apply_rs")
    else:
        check(lib().frhip_bn_bwd_apply(dt_of(y), _p(dout), _p(y), _p(coef[0]), _p(coef[1]), _p(coef[2]), ms, mb, _p(dy),
                                       rows, c, _s()), "frhip_bn_bwd_apply")
    return dy


def colsum_accumulate(x2d, out_accum):
    """out_accum[c] += sum_rows x2d[:, c]"""
    part = colstats(x2d)
    check(lib().frhip_sum_partials(_p(part), part.shape[0], x2d.shape[1], 0, _p(out_accum), _s()), "frhip_sum_partials")
    return out_accum


_DROP_GEN = None
_DROP_SEEN = None


def seed_dropout(seed):
    """pin the stream of dropout / stochastic-depth seeds (what torch.cuda.manual_seed is to the reference's nn.Dropout)"""
    global _DROP_GEN, _DROP_SEEN
    _DROP_GEN = torch.Generator()
    _DROP_GEN.manual_seed(int(seed) & ((1 << 63) - 1))
    _DROP_SEEN = torch.initial_seed()


def _drop_generator():
    """CPU generator of the dropout / stochastic-depth seeds, (re)seeded from torch.initial_seed() whenever that changes (a new
    torch.manual_seed(s)) or explicitly by seed_dropout().  NOT torch's default CPU generator: that one feeds PartialFC.sample's
    torch.rand(num_local) (/root/reference/nets/PartialFC.py:110), and the reference's nn.Dropout draws from the DEVICE generator -- a
    Swin / AlterNet step must leave the CPU stream exactly where the reference leaves it, or the sampled negative rows stop matching it seed
    for seed."""
    if _DROP_GEN is None or _DROP_SEEN != torch.initial_seed():
        seed_dropout(torch.initial_seed())
    return _DROP_GEN


def dropout_mask(shape, dtype, keep, device, seed=None):
    """mask of `shape`: 1/keep with probability keep, else 0 (one launch).  seed None: drawn from a generator of its own (_drop_generator)"""
    if seed is None:
        if torch.cuda.is_current_stream_capturing():
            # a captured graph would replay ONE host-drawn seed, i.e. the same mask every step: torch's device generator is graph-safe
            # (its Philox offset advances per replay), so the capture records the four-pass torch formulation instead
            return (torch.rand(shape, device=device) < keep).to(dtype) / keep
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=_drop_generator()).item())
    mask = torch.empty(shape, dtype=dtype, device=device)
    check(lib().frhip_dropout_mask(_DT[dtype], _p(mask), mask.numel(), float(keep), int(seed), _s()), "frhip_dropout_mask")
    return mask


def add_bias(x, bias):
    check(lib().frhip_add_bias(_p(x), _p(bias), x.shape[0], x.shape[1], _s()), "frhip_add_bias")
    return x


def cast_from_f32(src, dtype, out=None):
    out = torch.empty(src.shape, dtype=dtype, device=src.device) if out is None else out
    check(lib().frhip_cast_from_f32(_DT[dtype], _p(src), _p(out), src.numel(), _s()), "frhip_cast_from_f32")
    return out


def cast_to_f32(src, out=None):
    out = torch.empty(src.shape, dtype=torch.float32, device=src.device) if out is None else out
    check(lib().frhip_cast_to_f32(dt_of(src), _p(src), _p(out), src.numel(), _s()), "frhip_cast_to_f32")
    return out


# ------------------------------------------------------------------------------------------ stem
def stem_im2col(x_nchw, dtype, stride=1):
    b, c, h, w = x_nchw.shape
    assert c == 3 and x_nchw.dtype == torch.float32
    kp = 64 if dtype == torch.bfloat16 else 32
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    col = torch.empty((b * ho * wo, kp), dtype=dtype, device=x_nchw.device)
    check(lib().frhip_stem_im2col(_DT[dtype], _p(x_nchw), _p(col), b, h, w, stride, _s()), "frhip_stem_im2col")
    return col


def bn_relu_maxpool_fwd(y, st):
    b, h, w, c = y.shape
    hp, wp = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty((b, hp, wp, c), dtype=y.dtype, device=y.device)
    arg = torch.empty((b, hp, wp, c), dtype=torch.uint8, device=y.device)
    check(lib().frhip_bn_relu_maxpool_fwd(dt_of(y), _p(y), _p(st.scale), _p(st.shift), _p(out), _p(arg), b, h, w, c, _s()),
          "frhip_bn_relu_maxpool_fwd")
    return out, arg


def maxpool_bwd(dpool, arg, in_shape):
    b, h, w, c = in_shape
    da = torch.empty(in_shape, dtype=dpool.dtype, device=dpool.device)
    check(lib().frhip_maxpool_bwd(dt_of(dpool), _p(dpool), _p(arg), _p(da), b, h, w, c, _s()), "frhip_maxpool_bwd")
    return da


# ------------------------------------------------------------------------------------------ recompute-style stem
def stem_stats(x, wp):
    """BN-statistic partials [blocks, 2, 64] of conv3x3(x) (x fp32 NCHW, wp = pack_stem(w, dtype, kp=32))"""
    b, _, h, w = x.shape
    part = torch.empty((lib().frhip_stem_blocks(b, h, w), 2, 64), dtype=torch.float32, device=x.device)
    check(lib().frhip_stem_stats(dt_of(wp), _p(x), _p(wp), b, h, w, _p(part), _s()), "frhip_stem_stats")
    return part


def stem_fwd(x, wp, st):
    """maxpool(relu(bn(conv(x)))) -> (pooled [B,Hp,Wp,64], argmax uint8) without materialising the conv output"""
    b, _, h, w = x.shape
    hp, wq = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty((b, hp, wq, 64), dtype=wp.dtype, device=x.device)
    arg = torch.empty((b, hp, wq, 64), dtype=torch.uint8, device=x.device)
    check(lib().frhip_stem_fwd(dt_of(wp), _p(x), _p(wp), _p(st.scale), _p(st.shift), _p(out), _p(arg), b, h, w, _s()),
          "frhip_stem_fwd")
    return out, arg


def stem_gram(x, dtype):
    """{G = sum_p col col^T (27 x 27), s = sum_p col} of the stem's im2col columns, from the input batch alone (x rounded to `dtype`
    as the stem kernels round it): the data-only part of the stem's weight gradient (csrc/stem_algebra.hip)"""
    b, _, h, w = x.shape
    part = torch.empty((lib().frhip_stem_gram_blocks(b, h, w) + 1, 567), dtype=torch.float32, device=x.device)
    gram = torch.empty((lib().frhip_stem_gram_floats(),), dtype=torch.float32, device=x.device)
    check(lib().frhip_stem_gram(_DT[dtype], _p(x), b, h, w, _p(part), _p(gram), _s()), "frhip_stem_gram")
    return gram


def stem_bwd_coef(x, wp, dpool, arg, st, gamma, dgamma, dbeta, scratch=None, part=None):
    """the stem's BatchNorm backward: accumulates dgamma, dbeta (None: not wanted) and returns coef [3, 64] = (ca, cb, cc) of
    dy0 = ca * d + cb * y + cc.  part: [rows, 2, 64] partial sums { sum d, sum d * xhat } already reduced elsewhere (skips the
    recompute reduction pass)"""
    b, _, h, w = x.shape
    dev = x.device
    if part is None:
        part = torch.empty((lib().frhip_stem_blocks(b, h, w), 2, 64), dtype=torch.float32, device=dev)
        check(lib().frhip_stem_bwd_reduce(dt_of(wp), _p(x), _p(wp), _p(dpool), _p(arg), _p(st.mean), _p(st.invstd), _p(st.scale),
                                          _p(st.shift), b, h, w, _p(part), _s()), "frhip_stem_bwd_reduce")
    coef = torch.empty((3, 64), dtype=torch.float32, device=dev)
    if scratch is None:
        scratch = torch.empty((64 * 2 * 64,), dtype=torch.float32, device=dev)
    _bwd_finalize(part, scratch, 64, b * h * w, gamma, st, dgamma, dbeta, coef)
    return coef


def stem_bwd(x, wp, dpool, arg, st, gamma, dgamma, dbeta, dw27, scratch=None, part=None, gram=None, pooled=None):
    """backward of the stem given the gradient of the pooled map: accumulates dgamma, dbeta and dw27 [64, 27] (fp32); returns
    coef (stem_bwd_coef).  gram (+ pooled, the forward's output): stem_gram(x) -- the weight gradient then comes from the algebraic
    form (no conv recompute, no scatter) instead of the recompute kernel"""
    b, _, h, w = x.shape
    dev = x.device
    nb = lib().frhip_stem_blocks(b, h, w)
    coef = stem_bwd_coef(x, wp, dpool, arg, st, gamma, dgamma, dbeta, scratch, part)
    slabs = torch.empty((nb, 64, 32), dtype=torch.float32, device=dev)
    if gram is not None and pooled is not None:
        check(lib().frhip_stem_bwd_wgrad_gram(dt_of(wp), _p(x), _p(wp), _p(dpool), _p(pooled), _p(arg), _p(gram), _p(coef[0]), _p(coef[1]),
                                              _p(coef[2]), b, h, w, _p(slabs), _p(dw27), _s()), "frhip_stem_bwd_wgrad_gram")
        return coef
    check(lib().frhip_stem_bwd_wgrad(dt_of(wp), _p(x), _p(wp), _p(dpool), _p(arg), _p(coef[0]), _p(coef[1]), _p(coef[2]),
                                     _p(st.scale), _p(st.shift), b, h, w, _p(slabs), _p(dw27), _s()), "frhip_stem_bwd_wgrad")
    return coef


def _need_cuda(who, **tensors):
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("%s: %s must be a tensor on the GPU" % (who, name))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))


def stem_dx(x, wp, dpool, arg, pooled, coef, eval_mode=False):
    """image gradient of the stride-1 stem -> dx fp32 [B,3,H,W] (frhip_stem_dx).  x fp32 [B,3,H,W] NCHW, wp = pack_stem(w, dtype, kp=32),
    dpool / pooled [B,Hp,Wp,64] in wp's dtype, arg uint8 [B,Hp,Wp,64] (stem_fwd), coef [3,64] fp32 = (ca, cb, cc) of stem_bwd_coef.
    eval_mode: coef came from the eval-mode finalize (cb = cc = 0): the sparse form without the conv recompute"""
    _need_cuda("stem_dx", x=x, wp=wp, dpool=dpool, arg=arg, pooled=pooled, coef=coef)
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError("stem_dx: x must be fp32 [B,3,H,W], got %s %s" % (tuple(x.shape), x.dtype))
    b, _, h, w = x.shape
    pshape = (b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64)
    if wp.dtype not in _DT or tuple(wp.shape) != (64, 1, 1, 32):
        raise ValueError("stem_dx: wp must be pack_stem(w, dtype, kp=32) [64,1,1,32], got %s %s" % (tuple(wp.shape), wp.dtype))
    for name, t, dt in (("dpool", dpool, wp.dtype), ("pooled", pooled, wp.dtype), ("arg", arg, torch.uint8)):
        if tuple(t.shape) != pshape or t.dtype != dt:
            raise ValueError("stem_dx: %s must be %s %s, got %s %s" % (name, pshape, dt, tuple(t.shape), t.dtype))
    if tuple(coef.shape) != (3, 64) or coef.dtype != torch.float32:
        raise ValueError("stem_dx: coef must be fp32 [3,64]")
    dx = torch.empty((b, 3, h, w), dtype=torch.float32, device=x.device)
    cb, cc = (None, None) if eval_mode else (coef[1], coef[2])
    check(lib().frhip_stem_dx(dt_of(wp), _p(x), _p(wp), _p(dpool), _p(arg), _p(pooled), _p(coef[0]), _p(cb), _p(cc), b, h, w, _p(dx),
                              _s()), "frhip_stem_dx")
    return dx


def stem_dx_s2(dy0, wp, h, w):
    """image gradient of the stride-2 im2col stem: dx fp32 [B,3,h,w] = col2im(dy0 W^T) (frhip_stem_dx_s2).  dy0 [B,(h-1)/2+1,(w-1)/2+1,64]
    (the stem BatchNorm's input gradient), wp = pack_stem(w, dtype) [64,1,1,kp] in dy0's dtype"""
    _need_cuda("stem_dx_s2", dy0=dy0, wp=wp)
    if dy0.dim() != 4 or dy0.dtype not in _DT:
        raise ValueError("stem_dx_s2: dy0 must be [B,Ho,Wo,64] bf16 / fp32")
    b = dy0.shape[0]
    if tuple(dy0.shape) != (b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 64):
        raise ValueError("stem_dx_s2: dy0 %s does not match a %d x %d image" % (tuple(dy0.shape), h, w))
    if wp.dtype != dy0.dtype or wp.dim() != 4 or wp.shape[0] != 64 or wp.shape[3] < 27 or wp.shape[1] * wp.shape[2] != 1:
        raise ValueError("stem_dx_s2: wp must be pack_stem(w, dtype) [64,1,1,kp] in dy0's dtype")
    dx = torch.empty((b, 3, h, w), dtype=torch.float32, device=dy0.device)
    check(lib().frhip_stem_dx_s2(dt_of(dy0), _p(dy0), _p(wp), wp.shape[3], b, h, w, _p(dx), _s()), "frhip_stem_dx_s2")
    return dx


# ------------------------------------------------------------------------------------------ packs
def pack_wt(w_f32, dtype, out=None):
    """w [K,R,S,C] fp32 (physical) -> [C,R,S,K] dtype"""
    k, r, s, c = w_f32.shape
    out = torch.empty((c, r, s, k), dtype=dtype, device=w_f32.device) if out is None else out
    check(lib().frhip_pack_wt(_DT[dtype], _p(w_f32), _p(out), k, r * s, c, _s()), "frhip_pack_wt")
    return out


_WPREP = {}


def prep_conv_weights(weights, dtype):
    """weights: list of fp32 [K,R,S,C] (physical) conv weights -> ([K,R,S,C] dtype, [C,R,S,K] dtype) per tensor, all
    produced by ONE kernel launch into one arena that is reused from step to step (the pointer table is cached)."""
    import numpy as np
    key = (tuple(w.data_ptr() for w in weights), dtype)
    hit = _WPREP.get(key)
    if hit is None:
        dev = weights[0].device
        total = sum(w.numel() for w in weights)
        arena = torch.empty(2 * total, dtype=dtype, device=dev)
        es = arena.element_size()
        dt = np.dtype([("w", "<u8"), ("wc", "<u8"), ("wt", "<u8"), ("k", "<i4"), ("rs", "<i4"), ("c", "<i4"), ("tile_begin", "<i4")])
        tab = np.empty(len(weights), dtype=dt)
        outs, off, tiles = [], 0, 0
        for i, w in enumerate(weights):
            assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
            k, r, s, c = w.shape
            n = w.numel()
            wc = arena[off:off + n].view(k, r, s, c)
            wt = arena[off + n:off + 2 * n].view(c, r, s, k)
            tab[i] = (w.data_ptr(), wc.data_ptr(), wt.data_ptr(), k, r * s, c, tiles)
            tiles += ((k + 31) // 32) * ((c + 31) // 32) * r * s
            off += 2 * n
            outs.append((wc, wt))
        assert off * es == arena.numel() * es
        table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        if len(_WPREP) >= 8:
            _WPREP.clear()
        hit = _WPREP[key] = (table, len(weights), tiles, outs, arena, list(weights))
    table, n, tiles, outs, _, _ = hit
    check(lib().frhip_prep_conv_weights(_DT[dtype], _p(table), n, tiles, _s()), "frhip_prep_conv_weights")
    return outs


def transpose2d(x, out_dtype=None, out=None, pad_to=1):
    """x [rows][cols] -> [cols][ld] with ld = rows rounded up to pad_to (pad columns are zero)"""
    rows, cols = x.shape
    out_dtype = x.dtype if out_dtype is None else out_dtype
    ld = (rows + pad_to - 1) // pad_to * pad_to
    out = torch.empty((cols, ld), dtype=out_dtype, device=x.device) if out is None else out
    check(lib().frhip_transpose2d(dt_of(x), _DT[out_dtype], _p(x), _p(out), rows, cols, out.shape[1], _s()),
          "frhip_transpose2d")
    return out


def pack_stem(w_f32_k27, dtype, kp=None):
    k = w_f32_k27.shape[0]
    if kp is None:
        kp = 64 if dtype == torch.bfloat16 else 32
    out = torch.empty((k, 1, 1, kp), dtype=dtype, device=w_f32_k27.device)
    check(lib().frhip_pack_stem(_DT[dtype], _p(w_f32_k27), _p(out), k, 27, kp, _s()), "frhip_pack_stem")
    return out


def unpack_stem_grad(dwp, dw):
    k, kp = dwp.shape[0], dwp.numel() // dwp.shape[0]
    check(lib().frhip_unpack_stem_grad(_p(dwp), _p(dw), k, 27, kp, _s()), "frhip_unpack_stem_grad")


def fc_permute(w_f32, c, hw, dtype):
    nout = w_f32.shape[0]
    out = torch.empty((nout, hw * c), dtype=dtype, device=w_f32.device)
    check(lib().frhip_fc_permute(_DT[dtype], _p(w_f32), _p(out), nout, c, hw, _s()), "frhip_fc_permute")
    return out


def fc_unpermute_grad(dwp, dw, c, hw):
    check(lib().frhip_fc_unpermute_grad(_p(dwp), _p(dw), dw.shape[0], c, hw, _s()), "frhip_fc_unpermute_grad")


def gather_rows(src, index, out=None):
    n, d = index.numel(), src.shape[1]
    out = torch.empty((n, d), dtype=torch.float32, device=src.device) if out is None else out
    check(lib().frhip_gather_rows(_p(src), _p(index), _p(out), n, d, _s()), "frhip_gather_rows")
    return out


def scatter_rows(src, index, dst):
    check(lib().frhip_scatter_rows(_p(src), _p(index), _p(dst), index.numel(), src.shape[1], _s()), "frhip_scatter_rows")
    return dst


# ------------------------------------------------------------------------------------------ head
def l2norm_rows(x, dtype, eps=1e-12):
    rows, d = x.shape
    xh = torch.empty((rows, d), dtype=dtype, device=x.device)
    norms = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(lib().frhip_l2norm_rows(_DT[dtype], _p(x), _p(xh), _p(norms), rows, d, eps, _s()), "frhip_l2norm_rows")
    return xh, norms


def l2norm_bwd(dxhat, xhat, norms, out_scale=1.0):
    rows, d = dxhat.shape
    dx = torch.empty((rows, d), dtype=torch.float32, device=dxhat.device)
    check(lib().frhip_l2norm_bwd(dt_of(xhat), _p(dxhat), _p(xhat), _p(norms), _p(dx), rows, d, out_scale, _s()),
          "frhip_l2norm_bwd")
    return dx


def l2norm_bwd_norm(dxhat, xhat, norms, dnorm, out_scale=1.0):
    """l2norm_bwd plus the gradient of the norms themselves (dnorm [rows] fp32): dx = ((dxhat - xhat <dxhat, xhat>) / norm + dnorm xhat)
    out_scale in one launch (frhip_l2norm_bwd_norm)"""
    _need_f32("l2norm_bwd_norm", dxhat=dxhat, norms=norms, dnorm=dnorm)
    _need_cuda("l2norm_bwd_norm", xhat=xhat)
    rows, d = dxhat.shape
    if xhat.dtype not in _DT or xhat.shape != dxhat.shape or norms.numel() != rows or dnorm.numel() != rows:
        raise ValueError("l2norm_bwd_norm: xhat (bfloat16 or float32) must match dxhat %s and norms, dnorm hold one value per row, got %s %s, "
                         "%d, %d" % (tuple(dxhat.shape), xhat.dtype, tuple(xhat.shape), norms.numel(), dnorm.numel()))
    dx = torch.empty((rows, d), dtype=torch.float32, device=dxhat.device)
    check(lib().frhip_l2norm_bwd_norm(dt_of(xhat), _p(dxhat), _p(xhat), _p(norms), _p(dnorm), _p(dx), rows, d, out_scale, _s()),
          "frhip_l2norm_bwd_norm")
    return dx


def head_dw(dt, ehat, what, wnorm, out_scale=1.0):
    """class-centre gradient d_w [classes, 512] fp32 from dT [n, ldt], the normalised embeddings and centres and the centres' norms in one
    launch (frhip_head_dw), or None when the shape is not served (fp32 mode, d != 512): the caller then runs gemm_tn + l2norm_bwd"""
    n, d = ehat.shape
    classes = what.shape[0]
    if not lib().frhip_head_dw_ok(dt_of(ehat), n, classes, d):
        return None
    dw = torch.empty((classes, d), dtype=torch.float32, device=ehat.device)
    check(lib().frhip_head_dw(dt_of(ehat), _p(dt), dt.shape[1], _p(ehat), _p(what), _p(wnorm), _p(dw), n, classes, d, out_scale, _s()),
          "frhip_head_dw")
    return dw


MARGIN_ARCFACE, MARGIN_COSFACE = 0, 1          # frhip_margin_t.kind


class _MarginDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("easy", ctypes.c_int), ("s", ctypes.c_float), ("m", ctypes.c_float),
                ("filter_thr", ctypes.c_float)]


def _margin_desc(margin):
    """margin: (kind, easy, s, m, filter_thr), e.g. nets.ArcFace.Margin -> frhip_margin_t (passed by pointer)"""
    kind, easy, s, m, thr = margin
    return _MarginDesc(int(kind), int(bool(easy)), float(s), float(m), float(thr))


class _MarginRowsDesc(ctypes.Structure):
    _fields_ = [("s", ctypes.c_float), ("eps", ctypes.c_float), ("m_ang", ctypes.c_void_p), ("m_add", ctypes.c_void_p)]


def _is_rows(margin):
    """per-row margins (frhip_margin_rows_t), e.g. nets.ArcFace.RowMargins: fields s, eps and the device vectors m_ang, m_add [n] fp32"""
    return hasattr(margin, "m_ang")


def _margin_rows_desc(margin, n):
    for v in (margin.m_ang, margin.m_add):
        if v.dtype != torch.float32 or v.numel() != n:
            raise ValueError("per-row margins must be float32 vectors with one entry per row (%d), got %s %s"
                             % (n, v.dtype, tuple(v.shape)))
    return _MarginRowsDesc(float(margin.s), float(margin.eps), _p(margin.m_ang), _p(margin.m_add))


class _MarginCurrDesc(ctypes.Structure):
    _fields_ = [("s", ctypes.c_float), ("m", ctypes.c_float), ("thr", ctypes.c_void_p), ("t", ctypes.c_void_p)]


def _is_curr(margin):
    """CurricularFace (frhip_margin_curr_t), e.g. nets.ArcFace.CurrRows: fields s, m, the device vector thr [n] fp32 and the device scalar t"""
    return hasattr(margin, "thr")


def _margin_curr_desc(margin, n):
    _need_cuda("CurricularFace margin", thr=margin.thr, t=margin.t)
    if margin.thr.dtype != torch.float32 or margin.thr.numel() != n or not margin.thr.is_contiguous():
        raise ValueError("CurricularFace thresholds must be a contiguous float32 vector with one entry per row (%d), got %s %s"
                         % (n, margin.thr.dtype, tuple(margin.thr.shape)))
    if margin.t.dtype != torch.float32 or margin.t.numel() != 1:
        raise ValueError("CurricularFace's t must be one float32 element, got %s %s" % (margin.t.dtype, tuple(margin.t.shape)))
    return _MarginCurrDesc(float(margin.s), float(margin.m), _p(margin.thr), _p(margin.t))


class _MarginBceDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("s", ctypes.c_float), ("m", ctypes.c_float), ("m_neg", ctypes.c_float),
                ("w_pos", ctypes.c_float), ("w_neg", ctypes.c_float), ("bias", ctypes.c_void_p)]


def _is_bce(margin):
    """the sigmoid head (frhip_margin_bce_t), e.g. nets.ArcFace.BceMargin: fields kind, s, m, m_neg, w_pos, w_neg and the device scalar bias"""
    return hasattr(margin, "bias")


def _margin_bce_desc(margin):
    """The descriptor's values are judged by the library (one place, with its message); here only what ctypes cannot express"""
    _need_cuda("BCE margin", bias=margin.bias)
    if margin.bias.dtype != torch.float32 or margin.bias.numel() != 1:
        raise ValueError("the BCE head's bias must be one float32 element, got %s %s" % (margin.bias.dtype, tuple(margin.bias.shape)))
    return _MarginBceDesc(int(margin.kind), float(margin.s), float(margin.m), float(margin.m_neg), float(margin.w_pos),
                          float(margin.w_neg), _p(margin.bias))


def adaface_margins(norms, m, h, t_alpha, eps, batch_mean, batch_std, update):
    """AdaFace's per-row margins (m_ang, m_add) from the embedding norms [n] of the global batch in ONE launch (frhip_adaface_margins);
    update: the running batch_mean / batch_std (device scalars, fp32) are advanced in place first, else only read.  No host sync."""
    _need_cuda("adaface_margins", norms=norms, batch_mean=batch_mean, batch_std=batch_std)
    for nm, t in (("norms", norms), ("batch_mean", batch_mean), ("batch_std", batch_std)):
        if t.dtype != torch.float32:
            raise ValueError("adaface_margins: %s must be float32, got %s" % (nm, t.dtype))
    n = norms.numel()
    out = torch.empty((2, n), dtype=torch.float32, device=norms.device)
    check(lib().frhip_adaface_margins(_p(norms), n, m, h, t_alpha, eps, int(bool(update)), _p(batch_mean), _p(batch_std),
                                      _p(out[0]), _p(out[1]), _s()), "frhip_adaface_margins")
    return out[0], out[1]


def _need_f32(who, **tensors):
    _need_cuda(who, **tensors)
    for nm, t in tensors.items():
        if t.dtype != torch.float32:
            raise ValueError("%s: %s must be float32, got %s" % (who, nm, t.dtype))


def magface_margins(norms, l_a, u_a, l_m, u_m):
    """MagFace's per-row margins and regulariser from the embedding norms [n] of the global batch in ONE launch (frhip_magface_margins)
    -> (m_ang [n], m_add [n] = 0, reg [1] = mean of a / u_a^2 + 1 / a over a = clamp(norms, l_a, u_a)).  No host sync."""
    _need_f32("magface_margins", norms=norms)
    n = norms.numel()
    out = torch.empty((2, n), dtype=torch.float32, device=norms.device)
    reg = torch.empty((1,), dtype=torch.float32, device=norms.device)
    check(lib().frhip_magface_margins(_p(norms), n, l_a, u_a, l_m, u_m, _p(out[0]), _p(out[1]), _p(reg), _s()), "frhip_magface_margins")
    return out[0], out[1], reg


def magface_norm_grad(norms, packed, rmax, rsum, s, eps, l_a, u_a, l_m, u_m, lambda_g, gscale, upstream=None, out_scale=1.0):
    """d loss / d norms [n] of MagFace's loss (frhip_magface_norm_grad): norms [n] of the global batch, packed [ws, n, 3] the
    head_pack_stats blocks of all ranks, rmax / rsum [n] the global row statistics, gscale = 1 / n, upstream a device scalar or None"""
    tensors = dict(norms=norms, packed=packed, rowmax=rmax, rowsum=rsum)
    if upstream is not None:
        tensors["upstream"] = upstream
    _need_f32("magface_norm_grad", **tensors)
    n = norms.numel()
    if packed.dim() != 3 or packed.shape[1] != n or packed.shape[2] != 3 or rmax.numel() != n or rsum.numel() != n:
        raise ValueError("magface_norm_grad: packed must be [world_size, %d, 3] and rowmax, rowsum [%d], got %s, %s, %s"
                         % (n, n, tuple(packed.shape), tuple(rmax.shape), tuple(rsum.shape)))
    dnorm = torch.empty((n,), dtype=torch.float32, device=norms.device)
    check(lib().frhip_magface_norm_grad(_p(norms), _p(packed), packed.shape[0], n, _p(rmax), _p(rsum), s, eps, l_a, u_a, l_m, u_m,
                                        lambda_g, gscale, _p(upstream), out_scale, _p(dnorm), _s()), "frhip_magface_norm_grad")
    return dnorm


ELASTIC_KINDS = {"arc": MARGIN_ARCFACE, "cos": MARGIN_COSFACE}


def _elastic_args(who, n, std, seed, step):
    _need_cuda(who, step=step)
    if step.dtype != torch.int64 or step.numel() != 1:
        raise ValueError("%s: step must be one int64 element, got %s %s" % (who, step.dtype, tuple(step.shape)))
    if int(n) < 1 or not float(std) >= 0.0:
        raise ValueError("%s: needs n >= 1 rows and std >= 0, got n=%r std=%r" % (who, n, std))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF                      # the key is the seed's 64 bits; ctypes takes them as a signed value
    return int(n), seed - (1 << 64) if seed >> 63 else seed


def _elastic_kind(who, kind):
    if kind not in ELASTIC_KINDS and kind not in ELASTIC_KINDS.values():
        raise ValueError("%s: kind must be 'arc' (0) or 'cos' (1), got %r" % (who, kind))
    return ELASTIC_KINDS.get(kind, kind)


def elastic_margins(n, kind, mean, std, seed, step, update):
    """ElasticFace's per-row margins in ONE launch (frhip_elastic_margins): row i's draw from N(mean, std) by Philox at (seed, step, i),
    as m_ang (kind 'arc') or m_add (kind 'cos'), the other vector 0.  step: device scalar (int64); update: it is advanced by one in the
    same launch, else every margin is float(mean) and step is only read.  No host sync.  -> (m_ang [n], m_add [n])"""
    n, seed = _elastic_args("elastic_margins", n, std, seed, step)
    kind = _elastic_kind("elastic_margins", kind)
    out = torch.empty((2, n), dtype=torch.float32, device=step.device)
    check(lib().frhip_elastic_margins(n, kind, mean, std, seed, _p(step), int(bool(update)), _p(out[0]), _p(out[1]), _s()),
          "frhip_elastic_margins")
    return out[0], out[1]


def elastic_draws(n, mean, std, seed, step, update):
    """the bare draws g [n] of elastic_margins (frhip_elastic_draws), for elastic_assign"""
    n, seed = _elastic_args("elastic_draws", n, std, seed, step)
    g = torch.empty((n,), dtype=torch.float32, device=step.device)
    check(lib().frhip_elastic_draws(n, mean, std, seed, _p(step), int(bool(update)), _p(g), _s()), "frhip_elastic_draws")
    return g


def head_target_cos(ehat, what, labels_i32, subcenters=1):
    """tcos [n] fp32: the cosine of every row with the centre of its label, the maximum over the class's sub-centres (what: subcenters x
    classes rows, plane-major); exactly -2 where the label is -1 (frhip_head_target_cos)"""
    _need_cuda("head_target_cos", ehat=ehat, what=what, labels=labels_i32)
    k = _check_subcenters(what, subcenters)
    n, d = ehat.shape
    if (ehat.dtype not in _DT or what.dtype != ehat.dtype or what.shape[1] != d or labels_i32.dtype != torch.int32
            or labels_i32.numel() != n or not (ehat.is_contiguous() and what.is_contiguous() and labels_i32.is_contiguous())):
        raise ValueError("head_target_cos: ehat [n, d] and what [subcenters x classes, d] must be contiguous, of one dtype (bfloat16 or "
                         "float32), labels int32 [n]; got %s %s, %s %s, %s %s" % (ehat.dtype, tuple(ehat.shape), what.dtype,
                                                                                 tuple(what.shape), labels_i32.dtype, tuple(labels_i32.shape)))
    tcos = torch.empty((n,), dtype=torch.float32, device=ehat.device)
    check(lib().frhip_head_target_cos(dt_of(ehat), _p(ehat), _p(what), _p(labels_i32), n, what.shape[0] // k, d, k, _p(tcos), _s()),
          "frhip_head_target_cos")
    return tcos


def elastic_assign(tcos, g, kind):
    """ElasticFace+: tcos [world_size, n] (or [n]) target cosines of all ranks, g [n] draws -> (m_ang [n], m_add [n]): the row with the
    r-th largest cosine (maximum over ranks; ties in row order) gets the r-th smallest draw (frhip_elastic_assign; exact, n <= 65536)"""
    _need_f32("elastic_assign", tcos=tcos, g=g)
    kind = _elastic_kind("elastic_assign", kind)
    n = g.numel()
    tcos = tcos.reshape(1, -1) if tcos.dim() == 1 else tcos
    if tcos.dim() != 2 or tcos.shape[1] != n or g.dim() != 1 or not (tcos.is_contiguous() and g.is_contiguous()):
        raise ValueError("elastic_assign: tcos must be [world_size, %d] and g [%d], both contiguous, got %s, %s"
                         % (n, n, tuple(tcos.shape), tuple(g.shape)))
    nbytes = lib().frhip_elastic_assign_workspace(n)
    if nbytes <= 0:
        raise ValueError("elastic_assign: n = %d rows are not served (1 .. 65536)" % n)
    work = torch.empty((nbytes // 4,), dtype=torch.int32, device=g.device)
    out = torch.empty((2, n), dtype=torch.float32, device=g.device)
    check(lib().frhip_elastic_assign(_p(tcos), tcos.shape[0], n, _p(g), kind, _p(out[0]), _p(out[1]), _p(work), nbytes, _s()),
          "frhip_elastic_assign")
    return out[0], out[1]


def curricular_rows(tcos, m, alpha, t, update):
    """CurricularFace's per-row thresholds in ONE launch (frhip_curricular_rows): tcos [world_size, n] (or [n]) target cosines of all ranks
    (-2 where a rank does not own the row) -> thr [n] = cos(theta_y + m) of the merged cosine, +2 for a row nobody owns.  t: device scalar
    (fp32), the running mean of the target cosines; update: t <- alpha mean + (1 - alpha) t in the same launch, else t is not touched.
    No host sync."""
    _need_f32("curricular_rows", tcos=tcos, t=t)
    tcos = tcos.reshape(1, -1) if tcos.dim() == 1 else tcos
    if tcos.dim() != 2 or tcos.shape[1] < 1 or not tcos.is_contiguous() or t.numel() != 1:
        raise ValueError("curricular_rows: tcos must be [world_size, n] (contiguous, n >= 1) and t one element, got %s, %s"
                         % (tuple(tcos.shape), tuple(t.shape)))
    n = tcos.shape[1]
    thr = torch.empty((n,), dtype=torch.float32, device=tcos.device)
    check(lib().frhip_curricular_rows(_p(tcos), tcos.shape[0], n, float(m), float(alpha), int(bool(update)), _p(t), _p(thr), _s()),
          "frhip_curricular_rows")
    return thr


def head_sub_max():
    """the largest number of sub-centres per class the head kernels serve"""
    return lib().frhip_head_sub_max()


def _check_subcenters(what, subcenters):
    k = int(subcenters)
    if k < 1 or what.shape[0] % k:
        raise ValueError("subcenters=%d: what must hold subcenters x classes rows, plane-major; it has %d" % (k, what.shape[0]))
    return k


def _head_margin(margin, s, m, n, k):
    """-> (entry-point suffix, descriptor or None) of a head call: margin=None with one centre per class takes the (s, m) entry point"""
    if margin is None and k == 1:
        return "", None
    if margin is not None and _is_rows(margin):
        return "_rows", _margin_rows_desc(margin, n)
    if margin is not None and _is_curr(margin):
        return "_curr", _margin_curr_desc(margin, n)
    if margin is not None and _is_bce(margin):
        return "_bce", _margin_bce_desc(margin)
    return ("" if k > 1 else "_ex"), _margin_desc((MARGIN_ARCFACE, 0, s, m, 0.0) if margin is None else margin)


def head_fwd(ehat, what, labels_i32, s, m, margin=None, subcenters=1):
    """margin=None: ArcFace(s, m) (frhip_head_fwd); a (kind, easy, s, m, filter_thr) descriptor (frhip_head_fwd_ex); or per-row
    margins (s, eps, m_ang, m_add), e.g. nets.ArcFace.RowMargins (frhip_head_fwd_rows); or CurricularFace's (s, m, thr, t), e.g.
    nets.ArcFace.CurrRows (frhip_head_fwd_curr); or the sigmoid head's (kind, s, m, m_neg, w_pos, w_neg, bias), e.g. nets.ArcFace.BceMargin
    (frhip_head_fwd_bce): no softmax -- the result is then (ztarget, rowloss, rowdb[, tsub]), the rows' UNSCALED sums of the loss and
    bias-gradient terms, for bce_reduce / bce_merge.
    subcenters = K > 1 (frhip_head_fwd_sub / _sub_rows): what holds K x classes rows, plane-major (row k * classes + c); a class's cosine is
    the maximum over its K centres and the result gains tsub [n] int32, the winning centre of each row's target (-1: no target on this shard)."""
    k = _check_subcenters(what, subcenters)
    n, d = ehat.shape
    classes = what.shape[0] // k
    groups = lib().frhip_head_groups(classes)
    dev = ehat.device
    pm = torch.empty((groups, n), dtype=torch.float32, device=dev)
    ps = torch.empty((groups, n), dtype=torch.float32, device=dev)
    zt = torch.zeros((n,), dtype=torch.float32, device=dev)
    rmax = torch.empty((n,), dtype=torch.float32, device=dev)
    rsum = torch.empty((n,), dtype=torch.float32, device=dev)
    suffix, desc = _head_margin(margin, s, m, n, k)
    mg = (s, m) if desc is None else (ctypes.byref(desc),)
    head = (dt_of(ehat), _p(ehat), _p(what), _p(labels_i32), n, classes, d)
    if k > 1:
        tsub = torch.full((n,), -1, dtype=torch.int32, device=dev)
        name = "frhip_head_fwd_sub" + suffix
        check(getattr(lib(), name)(*head, k, *mg, _p(pm), _p(ps), _p(zt), _p(tsub), _p(rmax), _p(rsum), _s()), name)
        return zt, rmax, rsum, tsub
    name = "frhip_head_fwd" + suffix
    check(getattr(lib(), name)(*head, *mg, _p(pm), _p(ps), _p(zt), _p(rmax), _p(rsum), _s()), name)
    return zt, rmax, rsum


def head_rescale(rowsum, local_max, global_max):
    check(lib().frhip_head_rescale(_p(rowsum), _p(local_max), _p(global_max), rowsum.numel(), _s()), "frhip_head_rescale")


def head_target_prob(zt, labels_i32, rmax, rsum):
    q = torch.empty_like(zt)
    check(lib().frhip_head_target_prob(_p(zt), _p(labels_i32), _p(rmax), _p(rsum), _p(q), zt.numel(), _s()),
          "frhip_head_target_prob")
    return q


def head_pack_stats(zt, labels_i32, rmax, rsum, out=None):
    """[N,3] fp32 {local max, local sum-exp, target logit | -inf}: this rank's block of the one-exchange CE merge"""
    n = zt.numel()
    out = torch.empty((n, 3), dtype=torch.float32, device=zt.device) if out is None else out
    check(lib().frhip_head_pack_stats(_p(zt), _p(labels_i32), _p(rmax), _p(rsum), _p(out), n, _s()), "frhip_head_pack_stats")
    return out


def head_merge_stats(gathered):
    """gathered [ws,N,3] (all-gathered head_pack_stats blocks) -> global (rowmax, rowsum, q)"""
    ws, n, _ = gathered.shape
    buf = torch.empty((3, n), dtype=torch.float32, device=gathered.device)
    check(lib().frhip_head_merge_stats(_p(gathered), ws, n, _p(buf[0]), _p(buf[1]), _p(buf[2]), _s()), "frhip_head_merge_stats")
    return buf[0], buf[1], buf[2]


def head_loss(q):
    loss = torch.empty((1,), dtype=torch.float32, device=q.device)
    check(lib().frhip_head_loss(_p(q), q.numel(), _p(loss), _s()), "frhip_head_loss")
    return loss


_DT_TAIL = 256


def head_dw_sub(dt, ehat, what, wnorm, out_scale=1.0):
    """class-centre gradient [K x classes, d] fp32 from the K-plane dT [n, K, plane pitch] that head_bwd_dt(subcenters=K) returned (its
    allocation carries the tail the per-plane reads need: pass that tensor, not a copy): the kernels
    behind head_dw / gemm_tn + l2norm_bwd, once per plane, each on its plane's columns of dT (row pitch K x plane pitch) and its
    [classes, d] rows of the table"""
    n, k, ldp = dt.shape
    d = ehat.shape[1]
    classes = what.shape[0] // k
    dtype = dt_of(ehat)
    fused = bool(lib().frhip_head_dw_ok(dtype, n, classes, d))
    dw = torch.empty((k * classes, d), dtype=torch.float32, device=ehat.device)
    ws = None if fused else workspace(ehat.device)
    assert dt.is_cuda and dt.is_contiguous()
    behind = dt.untyped_storage().nbytes() - (dt.storage_offset() + dt.numel()) * dt.element_size()
    if behind < _DT_TAIL * dt.element_size():
        raise ValueError("head_dw_sub: dT must be the tensor head_bwd_dt(subcenters=K) returned: the per-plane reads need the %d zeroed "
                         "elements its allocation carries behind it" % _DT_TAIL)
    for j in range(k):
        rows = slice(j * classes, (j + 1) * classes)
        plane = dt.data_ptr() + j * ldp * dt.element_size()          # dT[:, j, :]: same row pitch, whole 16-byte vectors in
        if fused:
            check(lib().frhip_head_dw(dtype, plane, k * ldp, _p(ehat), _p(what[rows]), _p(wnorm[rows]), _p(dw[rows]), n, classes, d,
                                      out_scale, _s()), "frhip_head_dw")
        else:
            check(lib().frhip_gemm_tn_overwrite(dtype, plane, _p(ehat), _p(dw[rows]), n, classes, k * ldp, d, _p(ws),
                                                ws.numel() * 4, _s()), "frhip_gemm_tn_overwrite")
    if fused:
        return dw
    return l2norm_bwd(dw, what, wnorm, out_scale=out_scale)


def head_bwd_dt(ehat, what, labels_i32, s, m, rmax, rsum, gscale, upstream=None, transposed=False, margin=None, subcenters=1):
    """dT [n][classes padded]; transposed=True: also dTt [classes][n padded] from the same launch -> (dT, dTt).
    margin: as in head_fwd; the sigmoid head's (frhip_head_bwd_dt_bce) reads no row statistics: rmax, rsum are ignored (pass None).
    subcenters = K > 1 (what: K x classes rows, plane-major): dT is [n][K][classes padded] -- plane k holds d loss / d cos where centre k
    won its (row, class) and an exact 0 elsewhere, pad columns 0 -- and dTt is [K x classes][n padded], row k * classes + c."""
    k = _check_subcenters(what, subcenters)
    n, d = ehat.shape
    classes = what.shape[0] // k
    e = epv(ehat.dtype)
    ldp = (classes + e - 1) // e * e
    if k > 1:
        # head_dw_sub hands the TN GEMMs one plane at a time, as a pointer k * ldp columns into dT with dT's row pitch.  Those kernels fetch whole
        # column tiles (up to 256 columns, bounded by the pitch only) and drop what lies past their class count at the output; in the last row
        # of a later plane the tail of such a tile lies behind dT.  _DT_TAIL zeroed elements behind it keep those reads inside the allocation.
        flat = torch.empty((n * k * ldp + _DT_TAIL,), dtype=ehat.dtype, device=ehat.device)
        flat[n * k * ldp:].zero_()
        dt = flat[:n * k * ldp].view(n, k, ldp)
    else:
        dt = torch.empty((n, ldp), dtype=ehat.dtype, device=ehat.device)
    dtt, ldtt = None, 0
    if transposed:
        ldtt = (n + e - 1) // e * e
        dtt = torch.empty((k * classes, ldtt), dtype=ehat.dtype, device=ehat.device)
    suffix, desc = _head_margin(margin, s, m, n, k)
    mg = (s, m) if desc is None else (ctypes.byref(desc),)
    head = (dt_of(ehat), _p(ehat), _p(what), _p(labels_i32), n, classes, d)
    stats = (_p(rmax), _p(rsum), gscale, _p(upstream), _p(dt))
    if suffix == "_bce":
        stats = stats[2:]
    if k > 1:
        name = "frhip_head_bwd_dt_sub" + suffix
        check(getattr(lib(), name)(*head, k, *mg, *stats, k * ldp, ldp, _p(dtt), ldtt, _s()), name)
    else:
        name = "frhip_head_bwd_dt" + suffix
        check(getattr(lib(), name)(*head, *mg, *stats, ldp, _p(dtt), ldtt, _s()), name)
    return (dt, dtt) if transposed else dt


# ------------------------------------------------------------------------------------------ explicit-logit margin / CE
def margin_fwd(logits, labels_i64, s, m, kind):
    n, c = logits.shape
    tsave = torch.zeros((n,), dtype=torch.float32, device=logits.device)
    check(lib().frhip_margin_fwd(_p(logits), _p(labels_i64), n, c, s, m, kind, _p(tsave), _s()), "frhip_margin_fwd")
    return tsave


def margin_bwd(gout, labels_i64, tsave, s, m, kind):
    n, c = gout.shape
    gin = torch.empty_like(gout)
    check(lib().frhip_margin_bwd(_p(gout), _p(labels_i64), _p(tsave), n, c, s, m, kind, _p(gin), _s()), "frhip_margin_bwd")
    return gin


def margin_fwd_ex(logits, labels_i64, margin):
    """in place on logits [n, c] fp32 with a (kind, easy, s, m, filter_thr) descriptor -> (tsave, filter mask or None)"""
    n, c = logits.shape
    desc = _margin_desc(margin)
    tsave = torch.zeros((n,), dtype=torch.float32, device=logits.device)
    filt = torch.empty((n, (c + 63) // 64), dtype=torch.int64, device=logits.device) if desc.filter_thr > 0 else None
    check(lib().frhip_margin_fwd_ex(_p(logits), _p(labels_i64), n, c, ctypes.byref(desc), _p(tsave), _p(filt), _s()), "frhip_margin_fwd_ex")
    return tsave, filt


def margin_bwd_ex(gout, labels_i64, tsave, filt, margin):
    n, c = gout.shape
    desc = _margin_desc(margin)
    gin = torch.empty_like(gout)
    check(lib().frhip_margin_bwd_ex(_p(gout), _p(labels_i64), _p(tsave), _p(filt), n, c, ctypes.byref(desc), _p(gin), _s()),
          "frhip_margin_bwd_ex")
    return gin


def margin_fwd_rows(logits, labels_i64, margin):
    """out [n, c] = s x per-row margin of logits (margin: s, eps, m_ang, m_add); logits stay untouched (the backward reads them)"""
    n, c = logits.shape
    desc = _margin_rows_desc(margin, n)
    out = torch.empty_like(logits)
    check(lib().frhip_margin_fwd_rows(_p(logits), _p(labels_i64), n, c, ctypes.byref(desc), _p(out), _s()), "frhip_margin_fwd_rows")
    return out


def margin_bwd_rows(gout, logits, labels_i64, margin):
    n, c = gout.shape
    desc = _margin_rows_desc(margin, n)
    gin = torch.empty_like(gout)
    check(lib().frhip_margin_bwd_rows(_p(gout), _p(logits), _p(labels_i64), n, c, ctypes.byref(desc), _p(gin), _s()),
          "frhip_margin_bwd_rows")
    return gin


def margin_fwd_curr(logits, labels_i64, margin):
    """out [n, c] = s x CurricularFace of the cosines `logits` (margin: s, m, thr [n], t; frhip_margin_fwd_curr); logits stay untouched"""
    n, c = logits.shape
    _need_f32("margin_fwd_curr", logits=logits)
    desc = _margin_curr_desc(margin, n)
    out = torch.empty_like(logits)
    check(lib().frhip_margin_fwd_curr(_p(logits), _p(labels_i64), n, c, ctypes.byref(desc), _p(out), _s()), "frhip_margin_fwd_curr")
    return out


def margin_bwd_curr(gout, logits, labels_i64, margin):
    n, c = gout.shape
    _need_f32("margin_bwd_curr", gout=gout, logits=logits)
    desc = _margin_curr_desc(margin, n)
    gin = torch.empty_like(gout)
    check(lib().frhip_margin_bwd_curr(_p(gout), _p(logits), _p(labels_i64), n, c, ctypes.byref(desc), _p(gin), _s()),
          "frhip_margin_bwd_curr")
    return gin


def bce_reduce(rowloss, rowdb):
    """rowloss, rowdb [n] -> pair [2] fp32: this rank's UNSCALED sums, ONE one-workgroup launch in float64 (frhip_bce_reduce)"""
    _need_f32("bce_reduce", rowloss=rowloss, rowdb=rowdb)
    if rowloss.numel() != rowdb.numel() or not rowloss.is_contiguous() or not rowdb.is_contiguous():
        raise ValueError("bce_reduce: rowloss and rowdb must be contiguous vectors of one length, got %s, %s"
                         % (tuple(rowloss.shape), tuple(rowdb.shape)))
    pair = torch.empty((2,), dtype=torch.float32, device=rowloss.device)
    check(lib().frhip_bce_reduce(_p(rowloss), _p(rowdb), rowloss.numel(), _p(pair), _s()), "frhip_bce_reduce")
    return pair


def bce_merge(gathered, n_global):
    """gathered [ws, 2] (the all-gathered bce_reduce pairs; [2]: one rank) -> (loss [1], dbias [1]), folded in rank order in float64 and
    scaled by 1 / n_global (frhip_bce_merge)"""
    _need_f32("bce_merge", gathered=gathered)
    gathered = gathered.reshape(-1, 2)
    if not gathered.is_contiguous():
        raise ValueError("bce_merge: gathered must be contiguous")
    out = torch.empty((2,), dtype=torch.float32, device=gathered.device)
    check(lib().frhip_bce_merge(_p(gathered), gathered.shape[0], int(n_global), _p(out[0:1]), _p(out[1:2]), _s()), "frhip_bce_merge")
    return out[0:1], out[1:2]


def bce_fwd(logits, labels_i64, margin):
    """explicit cosines [n, c] fp32 -> (rowloss [n], rowdb [n]): the sigmoid head's UNSCALED row sums (frhip_bce_fwd); margin: BceMargin"""
    _need_f32("bce_fwd", logits=logits)
    n, c = logits.shape
    desc = _margin_bce_desc(margin)
    out = torch.empty((2, n), dtype=torch.float32, device=logits.device)
    check(lib().frhip_bce_fwd(_p(logits), _p(labels_i64), n, c, ctypes.byref(desc), _p(out[0]), _p(out[1]), _s()), "frhip_bce_fwd")
    return out[0], out[1]


def bce_bwd(logits, labels_i64, margin, gscale, upstream=None):
    """-> gin [n, c] = d (sum of the terms) / d logits x gscale x *upstream (frhip_bce_bwd)"""
    _need_f32("bce_bwd", logits=logits)
    n, c = logits.shape
    desc = _margin_bce_desc(margin)
    gin = torch.empty_like(logits)
    check(lib().frhip_bce_bwd(_p(logits), _p(labels_i64), n, c, ctypes.byref(desc), float(gscale), _p(upstream), _p(gin), _s()),
          "frhip_bce_bwd")
    return gin


def rows_max(x):
    n, c = x.shape
    out = torch.empty((n,), dtype=torch.float32, device=x.device)
    check(lib().frhip_rows_max(_p(x), n, c, _p(out), _s()), "frhip_rows_max")
    return out


def rows_exp_sum(x, rowmax):
    n, c = x.shape
    out = torch.empty((n,), dtype=torch.float32, device=x.device)
    check(lib().frhip_rows_exp_sum(_p(x), n, c, _p(rowmax), _p(out), _s()), "frhip_rows_exp_sum")
    return out


def rows_normalize(x, rowsum, labels_i64):
    n, c = x.shape
    pt = torch.empty((n,), dtype=torch.float32, device=x.device)
    check(lib().frhip_rows_normalize(_p(x), n, c, _p(rowsum), _p(labels_i64), _p(pt), _s()), "frhip_rows_normalize")
    return pt


def ce_grad(p, labels_i64, inv_n, upstream):
    n, c = p.shape
    check(lib().frhip_ce_grad(_p(p), n, c, _p(labels_i64), inv_n, _p(upstream), _s()), "frhip_ce_grad")
    return p


# ------------------------------------------------------------------------------------------ SwinV2 window attention
def winattn_fwd(qkv, bias, scale, b, h, w, heads, ws=7, shift=0):
    c = qkv.shape[1] // 3
    out = torch.empty((qkv.shape[0], c), dtype=qkv.dtype, device=qkv.device)
    check(lib().frhip_winattn_fwd(dt_of(qkv), _p(qkv), _p(bias), _p(scale), _p(out), b, h, w, c, heads, ws, shift, _s()),
          "frhip_winattn_fwd")
    return out


def winattn_bwd(qkv, dout, bias, scale, b, h, w, heads, ws=7, shift=0, want_colsum=False, dbias=None, dscale=None, qv_grads=None):
    """-> dqkv, dbias, dscale [, colsum fp32 [3c] = column sums of dqkv, or None when this dtype / kernel mode cannot fuse them].
    dbias / dscale given: the kernel ADDS into them (caller-zeroed accumulators) instead of fresh zero tensors.
    qv_grads = (dq_bias, dv_bias) fp32 [c] with want_colsum: the kernel adds the q / v column sums straight into these gradient
    accumulators (no [3c] temporary, no add passes) and the fourth result is True."""
    c = qkv.shape[1] // 3
    dqkv = torch.empty_like(qkv)
    ws_ = workspace(qkv.device)                  # per-workgroup partial sums of dbias / dscale / colsum, added in a fixed order
    dbias = torch.zeros_like(bias) if dbias is None else dbias
    dscale = torch.zeros_like(scale) if dscale is None else dscale
    if want_colsum:
        if qkv.dtype != torch.bfloat16 or not lib().frhip_set_winattn_mfma(-1):
            return winattn_bwd(qkv, dout, bias, scale, b, h, w, heads, ws, shift, dbias=dbias, dscale=dscale) + (None,)
        if qv_grads is not None:
            gq, gv = qv_grads
            assert gq.dtype == gv.dtype == torch.float32 and gq.numel() == gv.numel() == c and gq.is_contiguous() and gv.is_contiguous()
            check(lib().frhip_winattn_bwd_qvbias(dt_of(qkv), _p(qkv), _p(dout), _p(bias), _p(scale), _p(dqkv), _p(dbias), _p(dscale),
                                                 _p(gq), _p(gv), b, h, w, c, heads, ws, shift, _p(ws_), ws_.numel() * 4, _s()),
                  "frhip_winattn_bwd_qvbias")
            return dqkv, dbias, dscale, True
        colsum = torch.zeros(3 * c, dtype=torch.float32, device=qkv.device)
        check(lib().frhip_winattn_bwd_colsum(dt_of(qkv), _p(qkv), _p(dout), _p(bias), _p(scale), _p(dqkv), _p(dbias), _p(dscale),
                                             _p(colsum), b, h, w, c, heads, ws, shift, _p(ws_), ws_.numel() * 4, _s()),
              "frhip_winattn_bwd_colsum")
        return dqkv, dbias, dscale, colsum
    check(lib().frhip_winattn_bwd(dt_of(qkv), _p(qkv), _p(dout), _p(bias), _p(scale), _p(dqkv), _p(dbias), _p(dscale),
                                  b, h, w, c, heads, ws, shift, _p(ws_), ws_.numel() * 4, _s()), "frhip_winattn_bwd")
    return dqkv, dbias, dscale


def bias_gelu_fwd(y, bias, want_act):
    """y [rows, c] += bias in place; returns gelu(y) when want_act"""
    rows, c = y.shape
    act = torch.empty_like(y) if want_act else None
    check(lib().frhip_bias_gelu_fwd(dt_of(y), _p(y), _p(bias), _p(act), rows, c, _s()), "frhip_bias_gelu_fwd")
    return act


def gelu_bwd(da, h):
    dh = torch.empty_like(h)
    check(lib().frhip_gelu_bwd(dt_of(h), _p(da), _p(h), _p(dh), h.numel(), _s()), "frhip_gelu_bwd")
    return dh


# ------------------------------------------------------------------------------------------ verification metrics
def pair_score(e1, e2, labels_i64):
    n, d = e1.shape
    dev = e1.device
    scores = torch.empty((n,), dtype=torch.float64, device=dev)
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    hg = torch.zeros((100001,), dtype=torch.int32, device=dev)
    hi = torch.zeros((100001,), dtype=torch.int32, device=dev)
    check(lib().frhip_pair_score(_p(e1), _p(e2), _p(labels_i64), n, d, _p(scores), _p(idx), _p(hg), _p(hi), _s()),
          "frhip_pair_score")
    return scores, idx, hg, hi


def cross_score(e, labels_i64):
    """all pairs j < i of e [n,d] in the reference's order -> (scores f64 [P], pair labels f64 [P], hist idx i32 [P], hg, hi)"""
    n, d = e.shape
    dev = e.device
    pairs = n * (n - 1) // 2
    scores = torch.empty((pairs,), dtype=torch.float64, device=dev)
    plab = torch.empty((pairs,), dtype=torch.float64, device=dev)
    idx = torch.empty((pairs,), dtype=torch.int32, device=dev)
    hg = torch.zeros((100001,), dtype=torch.int32, device=dev)
    hi = torch.zeros((100001,), dtype=torch.int32, device=dev)
    check(lib().frhip_cross_score(_p(e), _p(labels_i64), n, d, _p(scores), _p(plab), _p(idx), _p(hg), _p(hi), _s()),
          "frhip_cross_score")
    return scores, plab, idx, hg, hi


CROSS_HIST_PAIRS_PER_LAUNCH = 1 << 30      # pairs per frhip_cross_hist launch: keeps one launch short on a shared device


def cross_hist_bands(n, pairs_per_launch=CROSS_HIST_PAIRS_PER_LAUNCH):
    """row boundaries [0, b1, ..., n] of the bands for cross_hist: each band [i0, i0 + h) holds about h i0 + h^2 / 2 <=
    pairs_per_launch pairs, h a multiple of the kernel's 128-row tile"""
    bounds, i0 = [0], 0
    while i0 < n:
        h = math.isqrt(i0 * i0 + 2 * pairs_per_launch) - i0
        rows = max(128, h // 128 * 128)
        i0 = min(n, i0 + rows)
        bounds.append(i0)
    return bounds


def cross_hist(e, labels_i64, bounds=None):
    """every pair j < i of e [n,d] counted without a pair list -> (hist_genuine, hist_imposter) int64 [100001] (the reference's
    bins) and (thr_genuine, thr_imposter) int64 [100002] (threshold slots, include/frhip.h frhip_cross_hist), on the device.
    `bounds`: row boundaries of the launches, 0 first and n last (default cross_hist_bands(n))."""
    n, d = e.shape
    dev = e.device
    bounds = cross_hist_bands(n) if bounds is None else list(bounds)
    if not bounds or bounds[0] != 0 or bounds[-1] != n or any(b1 < b0 for b0, b1 in zip(bounds, bounds[1:])):
        raise ValueError("cross_hist: bounds %r do not cover [0, %d) in order" % (bounds[:8], n))
    hg = torch.zeros((100001,), dtype=torch.int64, device=dev)
    hi = torch.zeros((100001,), dtype=torch.int64, device=dev)
    tg = torch.zeros((100002,), dtype=torch.int64, device=dev)
    ti = torch.zeros((100002,), dtype=torch.int64, device=dev)
    for i0, i1 in zip(bounds, bounds[1:]):
        check(lib().frhip_cross_hist(_p(e), _p(labels_i64), n, d, i0, i1, _p(hg), _p(hi), _p(tg), _p(ti), _s()), "frhip_cross_hist")
    return hg, hi, tg, ti


# ------------------------------------------------------------------------------------------ 1:N identification
GALLERY_TOPK_PAIRS_PER_LAUNCH = CROSS_HIST_PAIRS_PER_LAUNCH     # same reasoning: one launch stays short on a shared device


def gallery_topk_bands(p, g, pairs_per_launch=GALLERY_TOPK_PAIRS_PER_LAUNCH):
    """gallery row boundaries [0, b1, ..., g] of the launches of gallery_topk: bands of about pairs_per_launch / p rows, a
    multiple of the kernel's 128-row tile"""
    rows = max(128, pairs_per_launch // max(p, 1) // 128 * 128)
    return list(range(0, g, rows)) + [g]


def gallery_topk_workspace(p, k, device):
    """the split lists of one frhip_gallery_topk launch (frhip_gallery_topk_workspace bytes), one buffer per (device, stream)"""
    need = ctypes.c_int64(0)
    check(lib().frhip_gallery_topk_workspace(p, k, ctypes.byref(need)), "frhip_gallery_topk_workspace")
    key = ("gallery_topk", torch.device(device).index, _s())
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 8 < need.value:
        ws = _WORKSPACES[key] = torch.empty(max(1, need.value // 8), dtype=torch.float64, device=device)
    return ws


def gallery_topk(probe, gallery, k, exclude=None, bounds=None):
    """for every row of probe [P,d] fp32 the k best rows of gallery [G,d] fp32 -> (top_score float64 [P,k], top_index int64 [P,k]) on
    the device: frhip_cross_score's scores to the bit, score descending then gallery index ascending, unfilled slots -inf / -1
    (include/frhip.h frhip_gallery_topk).  `exclude` int64 [P]: the one gallery row probe i must not match (-1: none).  `bounds`:
    gallery row boundaries of the launches, 0 first and G last (default gallery_topk_bands(P, G))."""
    p, d = probe.shape
    g = gallery.shape[0]
    dev = probe.device
    assert gallery.dim() == 2 and gallery.shape[1] == d, "gallery_topk: probe [P,d] and gallery [G,d] expected"
    assert probe.dtype == torch.float32 and gallery.dtype == torch.float32, "gallery_topk: fp32 embeddings expected"
    assert exclude is None or (exclude.dtype == torch.int64 and exclude.numel() == p), "gallery_topk: exclude is int64 [P]"
    bounds = gallery_topk_bands(p, g) if bounds is None else list(bounds)
    if not bounds or bounds[0] != 0 or bounds[-1] != g or any(b1 < b0 for b0, b1 in zip(bounds, bounds[1:])):
        raise ValueError("gallery_topk: bounds %r do not cover [0, %d) in order" % (bounds[:8], g))
    ptrs = (_p(probe), _p(gallery), _p(exclude))
    k = int(k)
    top_score = torch.full((p, max(k, 0)), float("-inf"), dtype=torch.float64, device=dev)
    top_index = torch.full((p, max(k, 0)), -1, dtype=torch.int64, device=dev)
    ws = gallery_topk_workspace(p, k, dev)
    for g0, g1 in zip(bounds, bounds[1:]):
        check(lib().frhip_gallery_topk(*ptrs, p, g, d, k, g0, g1, _p(top_score), _p(top_index), _p(ws), ws.numel() * 8, _s()),
              "frhip_gallery_topk")
    return top_score, top_index


# ------------------------------------------------------------------------------------------ fp8 weight path (BASELINE cfg 5)
FP8_ACT_SCALE = 1.0        # static per-tensor scale of the fp8 activation copies: post-BatchNorm activations are O(1), e4m3 reaches 448


def quant_fp8_weights(w_f32):
    """fp32 [K, ...] (physical, contiguous) -> (fp8 bytes of the same shape, fp32 scale [K]): per-output-channel amax / 448"""
    k = w_f32.shape[0]
    rowlen = w_f32.numel() // k
    w8 = torch.empty(w_f32.shape, dtype=torch.uint8, device=w_f32.device)
    scale = torch.empty((k,), dtype=torch.float32, device=w_f32.device)
    check(lib().frhip_quant_fp8_weights(_p(w_f32), _p(w8), _p(scale), k, rowlen, _s()), "frhip_quant_fp8_weights")
    return w8, scale


_Q8W = {}


def quant_fp8_weights_multi(weights):
    """list of fp32 [K, ...] (physical, contiguous) weights -> [(fp8 bytes of the same shape, fp32 scale [K])], one launch into
    arenas that are reused from step to step (the pointer table is cached, like prep_conv_weights)"""
    import numpy as np
    key = tuple(w.data_ptr() for w in weights)
    hit = _Q8W.get(key)
    if hit is not None and any(r() is None for r in hit[6]):
        hit = None                                   # a weight of that entry is gone (its address was recycled): rebuild
    if hit is None:
        dev = weights[0].device
        bytes8 = torch.empty(sum(w.numel() for w in weights), dtype=torch.uint8, device=dev)
        scales = torch.empty(sum(w.shape[0] for w in weights), dtype=torch.float32, device=dev)
        dt = np.dtype([("w", "<u8"), ("w8", "<u8"), ("scale", "<u8"), ("k", "<i4"), ("rowlen", "<i4"), ("row_begin", "<i4"), ("pad", "<i4")])
        tab = np.zeros(len(weights), dtype=dt)
        outs, off, rows = [], 0, 0
        for i, w in enumerate(weights):
            assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
            k, n = w.shape[0], w.numel()
            assert (n // k) % 4 == 0 and off % 4 == 0
            w8 = bytes8[off:off + n].view(w.shape)
            sc = scales[rows:rows + k]
            tab[i] = (w.data_ptr(), w8.data_ptr(), sc.data_ptr(), k, n // k, rows, 0)
            off += n
            rows += k
            outs.append((w8, sc))
        # staged through a pinned slot with an async copy (a memcpy node when the first fp8 forward happens inside a graph capture, where a
        # blocking pageable copy is illegal), like optim._build_table; the slot lives as long as the cache entry
        raw = torch.from_numpy(tab.view(np.uint8).copy())
        pin = torch.empty(raw.numel(), dtype=torch.uint8, pin_memory=True)
        pin.copy_(raw)
        table = torch.empty(raw.numel(), dtype=torch.uint8, device=dev)
        table.copy_(pin, non_blocking=True)
        if len(_Q8W) >= 8:
            _Q8W.clear()
        # weights held by weak reference: the cache must not keep a dead model's parameters alive
        hit = _Q8W[key] = (table, len(weights), rows, outs, bytes8, scales, [weakref.ref(w) for w in weights], pin)
    table, n, rows, outs = hit[:4]
    check(lib().frhip_quant_fp8_weights_multi(_p(table), n, rows, _s()), "frhip_quant_fp8_weights_multi")
    return outs


def quant_fp8(x, inv_scale=1.0 / FP8_ACT_SCALE):
    x8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib().frhip_quant_fp8(dt_of(x), _p(x), _p(x8), x.numel(), inv_scale, _s()), "frhip_quant_fp8")
    return x8


def bn_apply_q8(y, st, relu=False, res=None, res_st=None):
    """bn_apply that also returns the fp8 copy of its output (the operand of the next fp8 GEMM)"""
    c = y.shape[-1]
    rows = y.numel() // c
    out = torch.empty_like(y)
    out8 = torch.empty(y.shape, dtype=torch.uint8, device=y.device)
    check(lib().frhip_bn_apply_q8(dt_of(y), _p(y), _p(st.scale), _p(st.shift), _p(res),
                                  _p(res_st.scale) if res_st is not None else None,
                                  _p(res_st.shift) if res_st is not None else None,
                                  int(relu), _p(out), _p(out8), 1.0 / FP8_ACT_SCALE, rows, c, _s()), "frhip_bn_apply_q8")
    return out, out8


def conv_fwd_fp8(x8, w8, wscale, stride, pad, want_stats=True):
    """x8 [N,H,W,C] fp8, w8 [K,R,S,C] fp8 + wscale [K] -> y bf16 [N,Ho,Wo,K], BatchNorm partials or None"""
    n, h, wd, c = x8.shape
    k, r, s, c2 = w8.shape
    assert c == c2 and x8.dtype == torch.uint8 and w8.dtype == torch.uint8
    ho, wo = conv_out_hw(h, wd, r, s, stride, pad)
    y = torch.empty((n, ho, wo, k), dtype=torch.bfloat16, device=x8.device)
    part = None
    if want_stats:
        rows = lib().frhip_fp8_conv_stat_rows(n * ho * wo, k, h, wd, c, r, s, stride, pad)
        part = torch.empty((rows, 2, k), dtype=torch.float32, device=x8.device)
    check(lib().frhip_conv_fwd_fp8(_p(x8), _p(w8), _p(wscale), FP8_ACT_SCALE, _p(y), _p(part), n, h, wd, c, k, r, s, stride, pad, _s()),
          "frhip_conv_fwd_fp8")
    return y, part


def linear_fwd_fp8(a8, w8, wscale, bias=None, want_stats=False):
    m, k = a8.shape
    n = w8.shape[0]
    out = torch.empty((m, n), dtype=torch.bfloat16, device=a8.device)
    part = None
    if want_stats:
        part = torch.empty((lib().frhip_fp8_stat_rows(m, n), 2, n), dtype=torch.float32, device=a8.device)
    check(lib().frhip_linear_fwd_fp8(_p(a8), _p(w8), _p(wscale), FP8_ACT_SCALE, _p(bias), _p(out), _p(part), m, n, k, _s()),
          "frhip_linear_fwd_fp8")
    return out, part
