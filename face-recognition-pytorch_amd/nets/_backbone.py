"""Shared host-side pieces of the frhip backbones (nets.resnet, nets.SwinV2): parameter containers with the
reference's names, and the forward / backward sequences of the parts every backbone of the reference shares --
stem (conv3x3 - BN - ReLU - MaxPool, /root/reference/nets/resnet.py:232-235 == nets/SwinV2.py:534-537), the IR
BasicBlock (nets/resnet.py:89-103) and the tail (bn2 - flatten - fc - bn3, nets/resnet.py:242-246).
Only orchestration lives here: every tensor op is a libfrhip kernel (frhip.ops)."""
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from frhip import ops
from frhip.optim import DEFERRED_SIDE, run_deferred_side  # noqa: F401  (DEFERRED_SIDE: the same list under its former name here)

_OVERLAP_WGRAD = os.environ.get("FRHIP_OVERLAP_WGRAD", "1") == "1"
# every weight gradient is followed by its own reduce launch.  Chaining the 3x3 weight gradients on 14 x 14 maps (each launch sums its
# predecessor's K-split slabs in its prologue, ops.conv_wgrad_chain) was measured slower and dropped: ResNet50 step, one box, alternating,
# 23.71 ms without / 23.85 with (and 23.85 / 24.24 with the hand-over behind the data-gradient up to 256 channels).
# The reduce launch (8 us alone, 50 - 65 us beside the main stream, which keeps the CUs' register files full) delays the next weight
# gradient so that it runs beside the HBM-bound BatchNorm-backward pass instead of beside the whole data-gradient: the chain removes 27
# launches and 1.4 ms of side-queue time and the main stream's convolutions slow down by more (in-step conv launch 145 -> 154 us).
_STEM_FUSED_REDUCE = True     # test hook; False: the stem's own recompute reduction pass
# True (default since the lean store epilogue, round 3): conv2's forward kernel forms a1 = relu(bn1(y1)) in LDS from y1 and writes it
# out on the way -- no BatchNorm-apply launch for bn1 in the forward pass, bit-identical tensors (-0.23 ms per step, three alternating
# pairs of 40-step runs on one box: 24.58 / 24.49 / 24.45 -> 24.28 / 24.31 / 24.21).  False (test hook; also wherever
# ops.conv_bnrelu_fusable says no): a1 is a BatchNorm-apply pass of its own.
# Never writing a1 (bn1-apply + ReLU folded into conv2's forward AND weight-gradient kernels, or re-formed on the side stream for the
# weight gradient) was measured slower and dropped: 29.5 ms fused vs 28.8 ms separate (ResNet50 step, B = 512, same box, two A/B rounds).
# The in-LDS transform is ~3.5 VALU operations per element in kernels whose matrix pipe already waits on instruction issue; in the
# weight gradient it costs more (+20 us per launch) than the 23-91 us HBM pass it removes wherever that pass is short.  DESIGN.md 4.8.
_FUSE_BN1 = True
# test hook: inference with the eval-mode BatchNorms folded into the store epilogues of the convolutions (False: separate BatchNorm-apply passes)
_EVAL_FOLD = True
# hand a weight gradient to the side stream BEFORE the data-gradient of the same dy is enqueued (the side stream waits for what
# the main stream holds at the hand-over): 27.16 -> 26.9 ms on the ResNet50 step.  One hand-over per block instead of one per
# weight gradient (fewer barrier packets, but conv2's weight gradient starts a data-gradient later) measured 27.3 -> 27.7: removed.
# ... except for layers of at most this many channels, whose weight gradient is handed over BEHIND the data-gradient that reads the
# same dy (on the wide early maps the BatchNorm-backward pass in front of each data-gradient is long and HBM-bound, and a weight
# gradient that starts with the data-gradient is done before the next such pass begins)
_WGRAD_LATE_MAXC = 64   # same-box A/B, two rounds: 26.15 / 26.13 (0) -> 26.06 / 26.04 (64), 26.11 / 26.16 (128), 26.40 / 26.37 ms (256)
_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32}


def compute_dtype(conf):
    """bf16 MFMA by default; conf.frhip_dtype or $FRHIP_DTYPE = 'fp32' selects the exact-fp32 validation mode."""
    name = getattr(conf, "frhip_dtype", None) or os.environ.get("FRHIP_DTYPE", "bf16")
    return _DTYPES[str(name).lower()]


# ------------------------------------------------------------------------------------------------- containers
class _Conv(nn.Module):
    """Parameter holder with the reference's name/shape ([K,C,R,S]); storage is channels_last = [K][R][S][C]."""

    def __init__(self, cin, cout, k, stride, bias=False, pad=None):
        super().__init__()
        self.cin, self.cout, self.k, self.stride = cin, cout, k, stride
        self.pad = (k - 1) // 2 if pad is None else pad
        w = torch.empty(cout, cin, k, k).contiguous(memory_format=torch.channels_last)
        self.weight = nn.Parameter(w)
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout))

    def physical(self):
        """fp32 [K,R,S,C] view of the weight (a copy only if someone replaced the channels_last storage)."""
        p = self.weight.data.permute(0, 2, 3, 1)
        return p if p.is_contiguous() else p.contiguous()


class _BN(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.eps, self.momentum = 1e-5, 0.1


class _Linear(nn.Module):
    def __init__(self, cin, cout, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin))
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout))


class BasicBlock(nn.Module):
    """conv3x3(inplanes->inplanes) - BN - ReLU - conv3x3(inplanes->planes, stride) - BN, + shortcut
    (reference nets/resnet.py:55-103).  Holds parameters only; the math runs in basic_block_forward/backward."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _Conv(inplanes, inplanes, 3, 1)
        self.bn1 = _BN(inplanes)
        self.conv2 = _Conv(inplanes, planes, 3, stride)
        self.bn2 = _BN(planes)
        self.downsample = downsample
        self.stride = stride


class Saved:
    pass


# ------------------------------------------------------------------------------------------------- gradients
def grad_like(p):
    return torch.zeros_like(p.data, memory_format=torch.preserve_format)


def phys_grad(g):
    if g is None:                   # input-gradient-only backward: no gradient arena
        return None
    pg = g.permute(0, 2, 3, 1)
    assert pg.is_contiguous()
    return pg


def flat_grads(params, device):
    """One zeroed fp32 arena for every parameter gradient of the step (a single fill instead of ~160), carved
    into views that have each parameter's own memory layout (channels_last for conv weights).
    -> (views {param: tensor}, arena, offsets {param: first element in the arena})

    The carving plan (size, stride, offset per parameter) is kept from step to step: building it costs ~0.5 ms of host time
    for a ResNet50 right where the host has no lead over the GPU (start of the backward pass); replaying it is one
    as_strided per parameter.  The view TENSORS are made afresh every step: autograd only adopts a gradient it holds the
    sole reference to (otherwise it clones it, and p.grad would stop aliasing the arena)."""
    key = (id(params[0]), id(params[-1]), len(params))
    plan = _ARENA_PLANS.get(key)
    if plan is not None and not all(a is b for a, b in zip(plan[2], params)):
        plan = None
    if plan is None:
        specs, off = [], 0
        for p in params:
            n = p.numel()
            if p.dim() == 4 and p.data.permute(0, 2, 3, 1).is_contiguous():
                k, c, r, s = p.shape
                specs.append((tuple(p.shape), (r * s * c, 1, s * c, c), off))
            elif p.data.is_contiguous():
                specs.append((tuple(p.shape), tuple(p.data.stride()), off))
            else:
                specs.append(None)                  # not in the arena: reduced on its own at join()
            off += n
        if len(_ARENA_PLANS) >= 8:
            _ARENA_PLANS.clear()
        offs = [None if sp is None else sp[2] for sp in specs]
        plan = _ARENA_PLANS[key] = (specs, off, list(params), offs)     # holds the parameters: their ids stay unique
    specs, total, _, offs = plan
    flat = torch.zeros(total, dtype=torch.float32, device=device)
    strided = flat.as_strided
    views = dict(zip(params, [grad_like(p) if sp is None else strided(sp[0], sp[1], sp[2]) for p, sp in zip(params, specs)]))
    return views, flat, dict(zip(params, offs))


_ARENA_PLANS = {}
_PREBUILT_ARENA = {}


_SIDE_STREAMS = {}


def _runs_beside(main, cand, ticks=50000):
    """True when a kernel on `cand` and a kernel on `main` execute at the same time (two 0.5-ms single-wave spins take about as
    long as one), False when the two streams share a hardware queue and serialise.  The first launch on a new stream creates its
    hardware queue (milliseconds) and the first cross-stream wait is slow too: one untimed round first."""
    from frhip._abi import check, lib
    e0, e1, ec = (torch.cuda.Event(enable_timing=True) for _ in range(3))

    def timed(both, t):
        torch.cuda.synchronize()
        e0.record(main)
        if both:
            check(lib().frhip_spin(t, cand.cuda_stream), "frhip_spin")
            ec.record(cand)
        check(lib().frhip_spin(t, main.cuda_stream), "frhip_spin")
        if both:
            main.wait_event(ec)
        e1.record(main)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    timed(True, 100)
    return timed(True, ticks) < 1.6 * timed(False, ticks)


def side_stream(device):
    """One long-lived side stream per device for the weight-gradient GEMMs -- one that really runs beside the main stream.
    HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4).  After RCCL and the c10d process group have
    taken theirs, a new stream can land on the queue of the main stream: everything then executes in enqueue order and the
    overlap is gone (ResNet50 step, 1-rank RCCL group: 31.3 ms against 26.1 ms).  So candidates are probed with two timed spin
    kernels and the first one that overlaps is kept."""
    main = torch.cuda.current_stream(device)
    key = (torch.device(device).index, main.cuda_stream)       # probed against THIS main stream; another one gets its own probe
    if key not in _SIDE_STREAMS:
        reuse = [v for k, v in _SIDE_STREAMS.items() if k[0] == key[0] and k[1] != "rejected" and v != main]
        tried = [reuse[0] if reuse else torch.cuda.Stream(device=device)]
        if torch.cuda.is_current_stream_capturing():              # no timing inside a graph capture: streams are graph branches there
            _SIDE_STREAMS[key] = tried[0]
            return tried[0]
        while not _runs_beside(main, tried[-1]) and len(tried) < 12:
            tried.append(torch.cuda.Stream(device=device))
        if not _runs_beside(main, tried[-1]):
            import warnings
            warnings.warn("frhip: no side stream runs concurrently with the main stream (all share its hardware queue); "
                          "weight gradients will not overlap -- raise GPU_MAX_HW_QUEUES")
            tried = tried[:1]
        _SIDE_STREAMS[key] = tried[-1]
        _SIDE_STREAMS[(key[0], "rejected", key[1])] = tried[:-1]      # keep them alive: later candidates get other queues
    return _SIDE_STREAMS[key]


# blocks of the backward pass to let go by before the side-stream work parked in frhip.optim (the head's early update) is launched
DEFER_EARLY_BLOCKS = 2        # 4 measured no faster


class BackwardCtx:
    """Gradient arena + the side stream on which weight gradients run + (data parallel) the gradient all-reduce.

    Weight gradients do not feed the rest of the backward chain, so they run on a side HIP stream.  Every tensor a
    side-stream kernel reads is kept referenced until the streams are joined again.

    Data parallel (`allreduce=True`, set by model.FR_PartialFC.Model on the wrapped encoder): the arena is laid out in
    parameter order and the backward pass finishes parameters in reverse order, so everything from the first parameter
    of the block just finished to the end of the arena is final.  `reduce_down_to(param)` averages that tail slice over
    the ranks IN PLACE with one RCCL all-reduce per >= 32 MB (no bucket copies: the arena is the bucket), issued behind
    the side stream so it overlaps the rest of the backward pass; join() waits for them.  This replaces torch DDP's
    reducer (the encoder's DDP wrapper is kept for its constructor broadcast and state_dict prefix, run under no_sync)."""

    MIN_BYTES = 32 << 20

    def __init__(self, params, device, allreduce=False, wgrad=True):
        """wgrad=False: backward for the input gradient alone (no parameter requires one) -- no arena (G(p) is None), no weight
        gradients, no side stream, no all-reduce"""
        pre = _PREBUILT_ARENA.pop(id(params), None)
        _PREBUILT_ARENA.clear()                         # at most one live forward pass per process
        self.wgrad_on = bool(wgrad)
        if self.wgrad_on:
            self.grads, self.flat, self.offsets = pre if pre is not None else flat_grads(params, device)
        else:
            self.grads, self.flat, self.offsets = {}, None, {}
        self.main = torch.cuda.current_stream()
        self.side = side_stream(device) if _OVERLAP_WGRAD and self.wgrad_on else None
        self.keep = []
        self.allreduce = self.wgrad_on and bool(allreduce) and dist.is_available() and dist.is_initialized()
        self.reduced_from = self.flat.numel() if self.wgrad_on else 0     # arena[reduced_from:] has been handed to RCCL
        self.works = []
        self.before_join = []                          # deferred gradient work (e.g. the batched position-bias backward)

    def G(self, p):
        return self.grads[p] if self.wgrad_on else None

    def on_side(self, fn, *tensors):
        """run fn() (weight-gradient work) on the side stream after everything enqueued so far on the main stream; nothing when no
        parameter gradient is wanted"""
        if not self.wgrad_on:
            return
        if self.side is None:
            fn()
            return
        self.keep.append(tensors)
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            fn()

    def wgrad(self, dy, x, gview, r, s, stride, pad):
        if not self.wgrad_on:
            return
        self.on_side(lambda: ops.conv_wgrad(dy, x, gview, r, s, stride, pad), dy, x, gview)

    def _reduce(self, lo, hi):
        if hi <= lo:
            return
        chunk = self.flat[lo:hi]
        # RCCL averages in the collective; other backends (gloo in tests) sum and join() scales
        op = dist.ReduceOp.AVG if dist.get_backend() == "nccl" else dist.ReduceOp.SUM
        if self.side is not None:                       # behind the weight gradients of this slice AND the main stream
            self.side.wait_stream(self.main)
            with torch.cuda.stream(self.side):
                if op != dist.ReduceOp.AVG:
                    self.side.synchronize()             # host-staged backends read the tensor from the host thread
                self.works.append(dist.all_reduce(chunk, op=op, async_op=True))
        else:
            if op != dist.ReduceOp.AVG:
                self.main.synchronize()
            self.works.append(dist.all_reduce(chunk, op=op, async_op=True))

    def reduce_down_to(self, param, force=False):
        """everything from `param` (in parameter order) to the end of the arena is final: hand it to RCCL"""
        if not self.allreduce:
            return
        lo = self.offsets.get(param)
        if lo is None or lo >= self.reduced_from:
            return
        if force or (self.reduced_from - lo) * 4 >= self.MIN_BYTES:
            self._reduce(lo, self.reduced_from)
            self.reduced_from = lo

    def run_deferred(self):
        """launch the side-stream work other modules parked for the backward pass (frhip.optim.DEFERRED_SIDE: the head's early
        parameter update)"""
        run_deferred_side()

    def join(self):
        self.run_deferred()
        for fn in self.before_join:
            fn()
        self.before_join = []
        if self.allreduce:
            self._reduce(0, self.reduced_from)
            self.reduced_from = 0
            for p, off in self.offsets.items():         # gradients that live outside the arena (unusual layouts)
                if off is None:
                    self.works.append(dist.all_reduce(self.grads[p], async_op=True,
                                                      op=dist.ReduceOp.AVG if dist.get_backend() == "nccl" else dist.ReduceOp.SUM))
        if self.side is not None:
            self.main.wait_stream(self.side)
        for w in self.works:
            w.wait()                                    # current (main) stream waits for the collective
        if self.allreduce and self.works and dist.get_backend() != "nccl":
            ws = dist.get_world_size()
            self.flat.mul_(1.0 / ws)
            for p, off in self.offsets.items():
                if off is None:
                    self.grads[p].mul_(1.0 / ws)
        self.works, self.keep = [], []
        return self.grads


class DataParallel(nn.Module):
    """Data-parallel wrapper of a frhip backbone with torch DDP's surface (`.module`, 'module.'-prefixed state_dict keys,
    parameters broadcast from rank 0 at construction) but without its bucketing reducer: the wrapped backbone averages
    its flat gradient arena in place with RCCL while its backward pass runs (BackwardCtx.reduce_down_to).  Stands where
    the reference has DistributedDataParallel(encoder, broadcast_buffers=False) (/root/reference/model/FR_PartialFC.py:92-96)."""

    def __init__(self, module, process_group=None):
        super().__init__()
        if not hasattr(module, "_backward_impl"):
            raise TypeError("DataParallel wraps the frhip backbones (nets.resnet / nets.SwinV2 / nets.AlterNet_SwinV2_FAN)")
        self.module = module
        module._frhip_allreduce = True
        if dist.is_available() and dist.is_initialized():
            with torch.no_grad():
                flat = torch.cat([p.data.reshape(-1) for p in module.parameters()] +
                                 [b.data.reshape(-1).float() for b in module.buffers()])
                dist.broadcast(flat, 0, group=process_group)          # same start on every rank (DDP does the same)
                off = 0
                for t in list(module.parameters()) + list(module.buffers()):
                    n = t.numel()
                    t.data.copy_(flat[off:off + n].view(t.shape).to(t.dtype))
                    off += n

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)


# ------------------------------------------------------------------------------------------------- forward pieces
_NBT_PENDING = None      # inside encoder_call: the num_batches_tracked counters to bump, in one multi-tensor add at the end
# inside EncoderFn.forward: False when no parameter wants a gradient (the forward pass then prepares no weight-gradient work, e.g. the
# stem's Gram pass); True otherwise and outside
_FWD_WGRAD = True
# inside an eval-mode EncoderFn.forward: the eval-mode BatchNorm states carry mean / invstd for the backward pass (bn_eval_state)
_EVAL_GRAD = False


def bn_forward_state(bn, part, count, training):
    if training:
        st = ops.bn_finalize(part, count, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var,
                             bn.momentum, bn.eps)
        if _NBT_PENDING is not None:
            _NBT_PENDING.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked += 1
        return st
    if _EVAL_GRAD:
        return ops.bn_eval_state(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.eps)
    return ops.bn_eval_affine(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.eps)


def stem_forward(net, x, training, sv):
    """conv3x3(3->64) - BN - ReLU - MaxPool(3,2,1) -> NHWC [B, H/2, W/2, 64].

    stride 1 (ResNet, SwinV2): recompute-style kernels -- the 64-channel conv output map (822 MB at B = 512) is never
    written: one pass computes the BN statistics, a second one recomputes the conv and pools.  stride 2 (AlterNet):
    im2col + GEMM, then fused BN + ReLU + MaxPool."""
    dt = net.dtype
    b, _, h, w = x.shape
    stride = net.conv1.stride
    if stride == 1:
        wp0 = ops.pack_stem(net.conv1.physical().reshape(64, 27), dt, kp=32)
        if training:
            st0 = bn_forward_state(net.bn1, ops.stem_stats(x, wp0), b * h * w, True)
        else:
            st0 = bn_forward_state(net.bn1, None, b * h * w, False)
        cur, arg0 = ops.stem_fwd(x, wp0, st0)
        if sv is not None:
            sv.x0, sv.wp0, sv.st0, sv.arg0, sv.col, sv.p0 = x, wp0, st0, arg0, None, cur
            sv.gram = None
            if training and _FWD_WGRAD:
                # the data-only part of the stem's weight gradient (csrc/stem_algebra.hip) needs x alone: it runs on the side stream
                # under the forward pass, and the backward pass then needs no recompute of the 112 x 112 x 64 conv map
                side = side_stream(x.device) if _OVERLAP_WGRAD else None
                if side is None:
                    sv.gram = ops.stem_gram(x, dt)
                else:
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        sv.gram = ops.stem_gram(x, dt)
                        sv.gram_done = torch.cuda.Event()
                        sv.gram_done.record(side)
        return cur
    col = ops.stem_im2col(x, dt, stride)
    h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
    wp0 = ops.pack_stem(net.conv1.physical().reshape(64, 27), dt)
    y0, part = ops.conv_fwd(col.view(b * h * w, 1, 1, col.shape[1]), wp0, 1, 0, want_stats=training)
    y0 = y0.view(b, h, w, 64)
    st0 = bn_forward_state(net.bn1, part, b * h * w, training)
    cur, arg0 = ops.bn_relu_maxpool_fwd(y0, st0)
    if sv is not None:
        sv.col, sv.y0, sv.st0, sv.arg0, sv.wp0, sv.x_hw = col, y0, st0, arg0, wp0, tuple(x.shape[2:])
    return cur


def stem_reduction_operands(net, sv):
    """(pooled map, stand-in BN state, ReLU flag) with which the generic BN-backward reduction -- fused into the epilogue of
    the kernel that produces the pooled map's gradient -- yields the STEM's reduction, or None (im2col stem).

    The stem's BN backward needs sum(d) and sum(d * xhat) over the 64-channel conv map, where d is the pooled gradient
    routed to the arg-max pixels and masked by the ReLU.  d is non-zero only at arg-max pixels, and there
    pooled = relu(gamma * xhat + beta): sum(d * xhat) = sum_pooled dpool * (pooled - beta) / gamma over pooled > 0 (pooled == 0:
    the ReLU blocks the gradient).  So a reduction over (dpool, pooled) with mean := beta, invstd := 1 / gamma and the mask
    pooled > 0 replaces a full recompute pass over the input (0.50 ms at B = 512).  1 / gamma is regularised,
    gamma / (gamma^2 + eps) with eps = (rounding noise of pooled - beta)^2: for a (near-)dead channel, |gamma| below the
    noise, the quotient would amplify rounding error without bound; it goes to zero instead."""
    if getattr(sv, "col", 0) is not None or getattr(sv, "p0", None) is None or not _STEM_FUSED_REDUCE:
        return None
    k = 2.0 ** -7 if sv.p0.dtype == torch.bfloat16 else 2.0 ** -20
    return sv.p0, ops.bn_standin_state(net.bn1.weight.data, net.bn1.bias.data, k, sv.st0.count), True


def stem_backward(net, sv, dout, bc, part=None):
    """part: the stem's BN-backward partial sums when the producer of dout already reduced them (stem_reduction_operands).
    sv.want_dx: the image gradient is requested -- it is left in sv.dx (fp32 [B,3,H,W])"""
    want_dx = getattr(sv, "want_dx", False)
    if sv.col is None:          # recompute-style stem
        dout = dout.contiguous()
        if bc.wgrad_on:
            gram = getattr(sv, "gram", None)
            if gram is not None and getattr(sv, "gram_done", None) is not None:
                torch.cuda.current_stream().wait_event(sv.gram_done)
                gram.record_stream(torch.cuda.current_stream())     # allocated on the side stream, read here
            coef = ops.stem_bwd(sv.x0, sv.wp0, dout, sv.arg0, sv.st0, net.bn1.weight.data, bc.G(net.bn1.weight),
                                bc.G(net.bn1.bias), phys_grad(bc.G(net.conv1.weight)).view(64, 27), part=part, gram=gram, pooled=sv.p0)
        else:
            coef = ops.stem_bwd_coef(sv.x0, sv.wp0, dout, sv.arg0, sv.st0, net.bn1.weight.data, None, None, part=part)
        if want_dx:
            sv.dx = ops.stem_dx(sv.x0, sv.wp0, dout, sv.arg0, sv.p0, coef, eval_mode=sv.st0.eval)
        return
    da0 = ops.maxpool_bwd(dout, sv.arg0, sv.y0.shape)
    dy0 = ops.bn_backward(da0, sv.y0, sv.st0, net.bn1.weight.data, bc.G(net.bn1.weight), bc.G(net.bn1.bias), relu_mask=True)
    if bc.wgrad_on:
        m, kp = sv.col.shape
        dwp0 = torch.zeros((64, 1, 1, kp), dtype=torch.float32, device=dout.device)
        ops.conv_wgrad(dy0.view(m, 1, 1, 64), sv.col.view(m, 1, 1, kp), dwp0, 1, 1, 1, 0)
        ops.unpack_stem_grad(dwp0, phys_grad(bc.G(net.conv1.weight)).view(64, 27))
    if want_dx:
        sv.dx = ops.stem_dx_s2(dy0, sv.wp0, *sv.x_hw)


def prepare_conv_weights(convs, dt):
    """{conv module: (bf16/fp32 [K,R,S,C], transposed [C,R,S,K])} for a list of _Conv modules, one kernel launch"""
    convs = list(convs)
    outs = ops.prep_conv_weights([c.physical() for c in convs], dt)
    return dict(zip(convs, outs))


def _operands(conv, dt, wprep):
    """(forward operand, data-gradient operand or None) of a conv: from the batched preparation when there is one"""
    if wprep is not None and conv in wprep:
        return wprep[conv]
    return ops.cast_from_f32(conv.physical(), dt), None


def use_fp8(conf):
    """conf.frhip_fp8 / $FRHIP_FP8 = 1: forward GEMMs with >= 128 input channels run on the fp8 MFMA path (BASELINE cfg 5)"""
    v = getattr(conf, "frhip_fp8", None)
    return bool(int(os.environ.get("FRHIP_FP8", "0"))) if v is None else bool(v)


class Fp8Ctx:
    """State of the fp8 weight path during ONE forward pass: the fp8 weight packs of the step (per-output-channel scales) and
    the fp8 copy of the activation tensor the last fused BatchNorm-apply pass wrote (the operand of the next GEMM)."""

    def __init__(self, weights):
        weights = list(weights)                        # w: fp32, physical [K, ...] with the reduction dims contiguous
        self.packs = dict(zip([m for m, _ in weights], ops.quant_fp8_weights_multi([w for _, w in weights]))) if weights else {}
        self._of, self._x8 = None, None

    @staticmethod
    def eligible(cin):
        return cin % 128 == 0                          # one K step of the fp8 kernels = 128 channels

    def put(self, x, x8):
        self._of, self._x8 = x, x8

    def take(self, x):
        """fp8 copy of x: the one its producer wrote, else a quantisation pass"""
        if self._of is x:
            return self._x8
        return ops.quant_fp8(x)


def basic_block_forward(blk, xin, dt, training, save, wprep=None, q8=None):
    """q8 (Fp8Ctx): convolutions whose input width is a multiple of 128 run on the fp8 MFMA kernels; the BatchNorm-apply
    passes that feed them write the fp8 operand copy themselves.  Everything saved for the backward pass stays as in the
    bf16 path (the backward kernels read the bf16 tensors)."""
    cin, planes = blk.conv1.cin, blk.conv2.cout
    if not training and not save and q8 is None and _EVAL_FOLD:
        # inference: the eval-mode BatchNorms are affine maps with fixed coefficients -- they ride in the store epilogues of the
        # convolutions that feed them (frhip_conv_fwd_affine); no BatchNorm-apply pass, no intermediate conv output tensor
        w1, _ = _operands(blk.conv1, dt, wprep)
        w2, _ = _operands(blk.conv2, dt, wprep)
        a1 = ops.conv_fwd_affine(xin, w1, bn_forward_state(blk.bn1, None, 0, False), 1, 1, relu=True)
        res = xin
        if blk.downsample is not None:
            dconv, dbn = blk.downsample[0], blk.downsample[1]
            wd, _ = _operands(dconv, dt, wprep)
            res = ops.conv_fwd_affine(xin, wd, bn_forward_state(dbn, None, 0, False), dconv.stride, 0)
        out = ops.conv_fwd_affine(a1, w2, bn_forward_state(blk.bn2, None, 0, False), blk.stride, 1, residual=res)
        return out, None
    f1 = q8 is not None and dt == torch.bfloat16 and Fp8Ctx.eligible(cin)      # conv1, conv2 and the shortcut conv all read cin channels
    fo = q8 is not None and dt == torch.bfloat16 and Fp8Ctx.eligible(planes)   # the block output feeds a GEMM of `planes` channels
    w1, w1t = _operands(blk.conv1, dt, wprep)
    x8 = q8.take(xin) if f1 else None
    if f1:
        y1, p1 = ops.conv_fwd_fp8(x8, *q8.packs[blk.conv1], 1, 1, want_stats=training)
    else:
        y1, p1 = ops.conv_fwd(xin, w1, 1, 1, want_stats=training)
    st1 = bn_forward_state(blk.bn1, p1, y1.numel() // y1.shape[3], training)
    w2, w2t = _operands(blk.conv2, dt, wprep)
    if f1:
        a1, a18 = ops.bn_apply_q8(y1, st1, relu=True)
        y2, p2 = ops.conv_fwd_fp8(a18, *q8.packs[blk.conv2], blk.stride, 1, want_stats=training)
    elif _FUSE_BN1 and ops.conv_bnrelu_fusable(y1, w2, blk.stride, 1):
        # conv2 forms a1 = relu(bn1(y1)) in LDS from y1 and writes it out on the way (the backward pass reads it): no BatchNorm-apply
        # launch, no second read of y1, the backward pass unchanged
        a1 = torch.empty_like(y1) if save else None
        y2, p2 = ops.conv_fwd_bnrelu(y1, st1, w2, blk.stride, 1, want_stats=training, act_out=a1)
    else:
        a1 = ops.bn_apply(y1, st1, relu=True)
        y2, p2 = ops.conv_fwd(a1, w2, blk.stride, 1, want_stats=training)
    st2 = bn_forward_state(blk.bn2, p2, y2.numel() // y2.shape[3], training)
    yd = std = wdt = None
    res, res_st = xin, None
    if blk.downsample is not None:
        dconv, dbn = blk.downsample[0], blk.downsample[1]
        wd, wdt = _operands(dconv, dt, wprep)
        if f1:
            yd, pd = ops.conv_fwd_fp8(x8, *q8.packs[dconv], dconv.stride, 0, want_stats=training)
        else:
            yd, pd = ops.conv_fwd(xin, wd, dconv.stride, 0, want_stats=training)
        std = bn_forward_state(dbn, pd, yd.numel() // yd.shape[3], training)
        res, res_st = yd, std
    if fo:
        out, out8 = ops.bn_apply_q8(y2, st2, res=res, res_st=res_st)
        q8.put(out, out8)
    else:
        out = ops.bn_apply(y2, st2, res=res, res_st=res_st)
    s = None
    if save:
        s = Saved()
        s.x, s.y1, s.st1, s.a1, s.y2, s.st2, s.yd, s.std = xin, y1, st1, a1, y2, st2, yd, std
        s.w1t, s.w2t, s.wdt = w1t, w2t, wdt
    return out, s


def basic_block_backward(blk, s, dout, dt, bc, part2=None, next_bn=None):
    """part2: BN-backward partial sums of (dout, s.y2) when the kernel that produced dout already reduced them.
    next_bn=(y, st[, relu]): the BatchNorm (relu: through a ReLU) that consumes the returned dx; its reduction is then fused
    into the epilogue of conv1's data-gradient and (dx, partial) is returned instead of dx."""
    G = bc.G
    dy2 = ops.bn_backward(dout, s.y2, s.st2, blk.bn2.weight.data, G(blk.bn2.weight), G(blk.bn2.bias), part=part2)
    shortcut, sc_stride = dout, 1
    if blk.downsample is not None:
        dconv, dbn = blk.downsample[0], blk.downsample[1]
        dyd = ops.bn_backward(dout, s.yd, s.std, dbn.weight.data, G(dbn.weight), G(dbn.bias))
        wdt = s.wdt if getattr(s, "wdt", None) is not None else ops.pack_wt(dconv.physical(), dt)
        if dconv.stride == 2:
            # a stride-2 1x1 conv only touches the even pixels: its data gradient is a plain GEMM on the compact grid, and
            # conv1's data-gradient epilogue adds it there (no zero-stuffed [N,H,W,C] tensor, 4x fewer rows)
            shortcut, sc_stride = ops.conv_dgrad(dyd, wdt, dyd.shape[:3] + (s.x.shape[3],), 1, 1, 1, 0), 2
        else:
            shortcut = ops.conv_dgrad(dyd, wdt, s.x.shape, 1, 1, dconv.stride, 0)
        bc.wgrad(dyd, s.x, phys_grad(G(dconv.weight)), 1, 1, dconv.stride, 0)
    w2t = s.w2t if getattr(s, "w2t", None) is not None else ops.pack_wt(blk.conv2.physical(), dt)
    # the BN1 (+ReLU) backward reduction over (da1, y1) rides in the epilogue of conv2's data-gradient
    def wgrad2():
        bc.wgrad(dy2, s.a1, phys_grad(G(blk.conv2.weight)), 3, 3, blk.stride, 1)
    # the side stream waits for what the main stream has enqueued at the moment of the hand-over: hand a weight gradient
    # over as soon as its operands are enqueued, i.e. BEFORE the data-gradient that reads the same dy
    early2 = dy2.shape[3] > _WGRAD_LATE_MAXC
    early1 = s.x.shape[3] > _WGRAD_LATE_MAXC
    if early2:
        wgrad2()
    da1, part1 = ops.conv_dgrad(dy2, w2t, s.y1.shape, 3, 3, blk.stride, 1, bnred=(s.y1, s.st1, True))
    if not early2:
        wgrad2()
    dy1 = ops.bn_backward(da1, s.y1, s.st1, blk.bn1.weight.data, G(blk.bn1.weight), G(blk.bn1.bias), relu_mask=True,
                          part=part1)
    w1t = s.w1t if getattr(s, "w1t", None) is not None else ops.pack_wt(blk.conv1.physical(), dt)
    if early1:
        bc.wgrad(dy1, s.x, phys_grad(G(blk.conv1.weight)), 3, 3, 1, 1)
    if next_bn is not None:
        dx = ops.conv_dgrad(dy1, w1t, s.x.shape, 3, 3, 1, 1, residual=shortcut,
                            bnred=(next_bn[0], next_bn[1], len(next_bn) > 2 and bool(next_bn[2])) + tuple(next_bn[3:]), residual_stride=sc_stride)
    else:
        dx = ops.conv_dgrad(dy1, w1t, s.x.shape, 3, 3, 1, 1, residual=shortcut, residual_stride=sc_stride)
    if not early1:
        bc.wgrad(dy1, s.x, phys_grad(G(blk.conv1.weight)), 3, 3, 1, 1)
    return dx


def tail_forward(net, cur, training, sv, dropout_mask=None, relu=False):
    """bn2 -> [relu] -> [dropout] -> flatten (NHWC order; fc columns permuted to match) -> fc -> bn3 (fp32 embeddings)"""
    dt = net.dtype
    bo, ho, wo, co = cur.shape
    rows = bo * ho * wo
    part = ops.colstats(cur.view(rows, co)) if training else None
    stt = bn_forward_state(net.bn2, part, rows, training)
    z = ops.bn_apply(cur, stt, relu=relu)
    if dropout_mask is not None:
        z = z * dropout_mask
    flat = z.view(bo, ho * wo * co)
    wfc = ops.fc_permute(net.fc.weight.data, co, ho * wo, dt)
    f = ops.gemm_nt_splitk(flat, wfc, net.fc.bias.data, splits=16)       # slabs added in split order: run-to-run identical
    part = ops.colstats(f) if training else None
    st3 = bn_forward_state(net.bn3, part, bo, training)
    emb = ops.bn_apply(f, st3)
    if sv is not None:
        sv.out4, sv.stt, sv.flat, sv.wfc, sv.f, sv.st3, sv.dropout_mask, sv.tail_relu = cur, stt, flat, wfc, f, st3, dropout_mask, relu
    return emb


def tail_backward(net, sv, d_emb, bc):
    dt = net.dtype
    G = bc.G
    df = ops.bn_backward(d_emb.contiguous().float(), sv.f, sv.st3, net.bn3.weight.data, G(net.bn3.weight), G(net.bn3.bias))
    # fc.bias only shifts the input of the training-mode bn3: its gradient (the column sums of df) is analytically zero
    # (1e-8-sized round-off in the reference) and stays at the arena's zero.  In eval mode bn3 is a fixed affine map: it is not.
    if sv.st3.eval and bc.wgrad_on:
        ops.colsum_accumulate(df, G(net.fc.bias))
    dft = ops.cast_from_f32(df, dt)
    b, kfc = sv.flat.shape
    wfct = ops.transpose2d(sv.wfc)                                  # [25088][512]
    dflat = ops.gemm_nt(dft, wfct)                                  # [B][25088]
    if bc.wgrad_on:
        dwp = torch.empty((net.emd_size, kfc), dtype=torch.float32, device=d_emb.device)
        ops.gemm_tn(dft, sv.flat, dwp, overwrite=True)              # 51 MB: stored once (no zero fill + atomic pass)
        co = sv.out4.shape[3]
        ops.fc_unpermute_grad(dwp, G(net.fc.weight), co, kfc // co)
    dz = dflat.view(sv.out4.shape)
    if sv.dropout_mask is not None:
        dz = dz * sv.dropout_mask
    return ops.bn_backward(dz, sv.out4, sv.stt, net.bn2.weight.data, G(net.bn2.weight), G(net.bn2.bias),
                           relu_mask=sv.tail_relu)


class EncoderFn(torch.autograd.Function):
    """The whole backbone as ONE autograd node: forward keeps what backward needs, backward runs the hand-written
    gradient kernels and returns every parameter gradient."""

    @staticmethod
    def forward(ctx, net, x, *params):
        global _FWD_WGRAD, _EVAL_GRAD
        # parameter gradients are computed when any parameter wants one (a partly frozen net's other gradients are discarded);
        # none wanted (net.requires_grad_(False), the usual adversarial-attack setup): backward for the image gradient alone
        wgrad = any(ctx.needs_input_grad[2:])
        training = net.training
        _FWD_WGRAD, _EVAL_GRAD = wgrad, not training
        try:
            # eval mode: the unfolded forward path (the folded one, _EVAL_FOLD, keeps none of what the backward pass reads) with
            # eval-mode BatchNorm states that carry the running statistics; dropout and stochastic depth are the identity
            emb, sv = net._forward_impl(x, training, True)
        finally:
            _FWD_WGRAD, _EVAL_GRAD = True, False
        sv.wgrad, sv.want_dx = wgrad, bool(ctx.needs_input_grad[1])
        ctx.net, ctx.sv, ctx.params = net, sv, params
        # the gradient arena of the backward pass, carved NOW: the forward pass has just been enqueued, so the host is ahead
        # of the GPU here; at the start of the backward pass (behind a short sampled head) it is not, and the ~1 ms of
        # host time the 160 views cost would be GPU idle time
        _PREBUILT_ARENA.clear()                         # at most one: a forward pass that is never differentiated leaks nothing
        if wgrad:
            _PREBUILT_ARENA[id(params)] = flat_grads(params, x.device)
        return emb

    @staticmethod
    def backward(ctx, d_emb):
        sv = ctx.sv
        grads = ctx.net._backward_impl(sv, d_emb, ctx.params)
        dx = getattr(sv, "dx", None) if sv.want_dx else None
        ctx.sv = None
        return (None, dx) + tuple(grads.get(p) for p in ctx.params)


def encoder_call(net, x):
    """training mode under grad mode: the autograd node (EncoderFn).  Eval mode: the autograd node when grad mode is on and x or a
    parameter requires a gradient, else the inference path (folded BatchNorms)."""
    differentiate = torch.is_grad_enabled() and (net.training or x.requires_grad or
                                                 any(p.requires_grad for p in net.parameters()))
    if differentiate and not net.training and getattr(net, "fp8", False):
        raise NotImplementedError("frhip backbone: eval-mode differentiation of an fp8 model (frhip_fp8 / FRHIP_FP8=1) is not "
                                  "implemented; run it under torch.no_grad(), or build the model without fp8")
    if not x.is_cuda:
        raise RuntimeError("frhip backbone: input must live on the MI355X; there is no CPU path "
                           "(the CPU restatement lives in oracle/ and is test-only)")
    x = x.contiguous().float()
    global _NBT_PENDING
    _NBT_PENDING = []
    try:
        if differentiate:
            out = EncoderFn.apply(net, x, *[p for p in net.parameters()])
        else:
            out, _ = net._forward_impl(x, net.training, False)
        if _NBT_PENDING:
            torch._foreach_add_(_NBT_PENDING, 1)        # ~60 one-element increments as one launch
    finally:
        _NBT_PENDING = None
    return out
