"""Poisoned allocations for the kernel and step tests.  TEST-ONLY.

Nearly every output of the native library lands in memory that Python allocated with torch.empty and never initialised
(frhip/ops.py, nets/*, model/*).  In a fresh process that memory is mostly zeros, so a kernel that reads an element nobody wrote -- a
partial-sum row past the last one stored, a K-split slab no split filled, the pad columns of a pitched operand -- goes unnoticed.

`poisoned_empty(pattern)` makes torch.empty, torch.empty_like and torch.Tensor.new_empty hand out FLOATING-POINT tensors filled with
`pattern` while it is active.  Integer and bool tensors (labels, weight_index, pooling arg-max, sampled indices) are left as they are:
a poisoned index would be an out-of-bounds access, so integer buffers are reviewed by reading the code instead.  The C++ side allocates
no device memory apart from module globals it writes before it reads them, so this reaches every buffer a kernel is handed.

Patterns (PATTERNS): nan catches arithmetic use of an unwritten element; 3e38 catches reads that pass through fmaxf, compares and selects,
where a NaN can slip by; 0.75 is a plausible value that only biases a sum -- the kind of read that drifts a statistic by a few percent
without ever producing a non-finite number.

`reset_frhip_caches()` drops the module-level buffer caches of frhip / nets so that the next call allocates them again -- under the
poison, when it is active."""
import contextlib
import math

import torch

PATTERNS = (float("nan"), 3e38, 0.75)
PATTERN_IDS = ("nan", "3e38", "0.75")


def _fill(t, pattern):
    if isinstance(t, torch.Tensor) and t.is_floating_point() and t.numel() > 0:
        if math.isfinite(pattern):
            pattern = min(pattern, torch.finfo(t.dtype).max)      # 3e38 in a dtype that cannot hold it (fp16): its largest finite value
        with torch.no_grad():
            t.fill_(pattern)
    return t


@contextlib.contextmanager
def poisoned_empty(pattern):
    """while active: floating-point results of torch.empty / torch.empty_like / Tensor.new_empty hold `pattern`.  Nests (the innermost
    pattern wins); the previous functions are restored on exit, also when the body raises."""
    pattern = float(pattern)
    prev_empty, prev_like, prev_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def empty(*args, **kwargs):
        return _fill(prev_empty(*args, **kwargs), pattern)

    def empty_like(*args, **kwargs):
        return _fill(prev_like(*args, **kwargs), pattern)

    def new_empty(self, *args, **kwargs):
        return _fill(prev_new(self, *args, **kwargs), pattern)

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield pattern
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = prev_empty, prev_like, prev_new


def holds(t, pattern):
    """True when every element of t equals `pattern` as rounded to t's dtype (nan: every element is a NaN)"""
    if t.numel() == 0:
        return False
    if math.isnan(pattern):
        return bool(torch.isnan(t).all())
    return bool((t == torch.tensor(pattern, dtype=t.dtype, device=t.device)).all())


def assert_poison_applies(pattern, dtype, device="cuda"):
    """the probe every poisoned case runs before its call: a fresh torch.empty of `dtype` must hold the pattern, or the case fails
    instead of passing on memory that was never poisoned"""
    probe = torch.empty((257,), dtype=dtype, device=device)
    assert holds(probe, pattern), "poison %r did not apply to a torch.empty of %s" % (pattern, dtype)


def reset_frhip_caches():
    """drop every module-level device-buffer cache of frhip / nets, so that the next call allocates it again through torch.empty (under
    an active poisoned_empty: filled with the pattern).  Caches of host-side facts (shape predicates, side streams, carving plans) stay."""
    from frhip import ops, optim
    ops._WORKSPACES.clear()          # split-K workspace (slabs of the weight-gradient GEMMs, gemm_nt_splitk)
    ops._CHAIN_SLABS.clear()         # slab pair of the chained 14 x 14 weight gradients
    ops._WPREP.clear()               # arena of the per-step bf16 weight packs + its pointer table
    ops._Q8W.clear()                 # fp8 weight packs + scales
    del optim.DEFERRED_SIDE[:]       # head update parked for a backward pass
    try:
        from nets import _backbone
    except ImportError:
        return
    _backbone._PREBUILT_ARENA.clear()    # gradient arena carved during the forward pass (zero-filled, but dropped all the same)
