"""Every kernel of the recompute-style stem (csrc/stem_fused.hip, csrc/stem_algebra.hip) on the GPU, on operands whose every element
bf16 holds and whose every sum fp32 holds exactly, at every tile edge of every kernel.

tests/stem_cases.py has the cases -- one-pixel, one-row and one-column maps, both sides of the 4 x 28 pooled tile of the forward and
backward kernels, of the 16-pixel step and the 8-row band of the statistics kernel, of the 16 x 16 tile of the image gradient and of the
8 x 8 pooled tile of the gather, a batch that takes the grid-stride loops past both grid caps, the widest rows -- and the float64
reference; tests/test_stem_cases_cpu.py pins the value bounds and that each case has ties, pooled zeros, pre-activations of exactly 0 and
arg-max pixels in the neighbour tiles.  Here every entry point runs per case and element type and must EQUAL the reference
(torch.equal, no tolerance, no element left out), twice with identical bits.  The backward entry points take the arg-max bytes and the
pooled map from the reference, so a forward defect cannot hide a backward one; one test per element type chains the device's own forward
into them.  Every buffer lies between canaries in memory poisoned through tests/poison.py (NaN; 0xFF for bytes), scratch at exactly its
documented size: blocks x 2 x 64, blocks x 2048 and (gram blocks + 1) x 567 floats."""
import contextlib

import pytest
import torch

import stem_cases as sc

pytestmark = pytest.mark.gpu

FULL = [(case.name, dt) for case in sc.FULL for dt in case.dtypes]
STATS = FULL + [(case.name, dt) for case in sc.CASES if case.only == "stats" for dt in case.dtypes]
GRAM = FULL + [(case.name, dt) for case in sc.CASES if case.only == "gram" for dt in case.dtypes]
# the backward forms: fp32 always gathers; bf16 scatters by default and gathers under frhip_set_stem_scatter(0)
FORMS = [(name, dt, form) for name, dt in FULL for form in (("gather",) if dt == "fp32" else ("scatter", "gather"))]
VECTORS = ("scale", "shift", "mean", "invstd", "ca", "cb", "cc")


def _api():
    from frhip import ops
    from frhip._abi import check, lib
    return ops, check, lib()


@contextlib.contextmanager
def backward_form(form, dt):
    _, _, lib = _api()
    old = lib.frhip_set_stem_scatter(0 if form == "gather" and dt == "bf16" else 1)
    try:
        yield
    finally:
        lib.frhip_set_stem_scatter(old)


def same(got, want, what):
    got, want = got.cpu(), want.to(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        g, w = got.double(), want.double()
        wrong = (g != w) | torch.isnan(g)
        raise AssertionError("%s: %d of %d elements differ, largest difference %r, first at %r: got %r, want %r" % (
            what, int(wrong.sum()), want.numel(), float((g - w).abs().nan_to_num(float("inf")).max()),
            tuple(wrong.nonzero()[0].tolist()), float(g[wrong][0]), float(w[wrong][0])))


def same_bits(a, b, what):
    for key in a:
        assert torch.equal(a[key].contiguous().view(torch.uint8), b[key].contiguous().view(torch.uint8)), (what, key, "differs from run to run")


def twice(run, what):
    first, second = run(), run()
    same_bits(first, second, what)
    return first


class Launch:
    """the guarded device operands of one launch of a case: x, the packed weights, the per-channel vectors, and on demand the pooled
    gradient, the arg-max bytes and the pooled map (from the reference unless the caller hands in the device's own)"""

    def __init__(self, name, dt, arg=None, pooled=None):
        self.case, self.data, self.ref = sc.BY_NAME[name], sc.operands(name), sc.reference(name)
        self.dtype, self.mem = sc.DTYPES[dt], sc.Guarded()
        self.ops, self.check, self.lib = _api()
        self.code = self.ops._DT[self.dtype]
        self.x = self.mem.put(self.data["x"], torch.float32, "x")
        self.wp = self.mem.put(sc.packed_weights(self.data["w"], self.dtype), self.dtype, "wp")
        self.vec = {key: self.mem.put(self.data[key], torch.float32, key) for key in VECTORS}
        self.geom = (self.case.b, self.case.h, self.case.w)
        self.blocks = self.lib.frhip_stem_blocks(*self.geom)
        self._arg, self._pooled = arg, pooled

    def dpool(self):
        return self.mem.put(self.data["dpool"], self.dtype, "dpool")

    def arg(self):
        return self.mem.put(self.ref["arg"] if self._arg is None else self._arg, torch.uint8, "argmax")

    def pooled(self):
        return self.mem.put(self.ref["pooled"] if self._pooled is None else self._pooled, self.dtype, "pooled")

    def dw(self):
        return self.mem.put(self.data["dw0"], torch.float32, "dw")

    def p(self, t):
        return self.ops._p(t)

    def done(self, rc, what, **outputs):
        self.check(rc, what)
        torch.cuda.synchronize()
        self.mem.check()
        return {key: t.cpu() for key, t in outputs.items()}


def run_stats(name, dt):
    L = Launch(name, dt)
    part = L.mem.out((L.blocks, 2, 64), torch.float32, "partial")
    return L.done(L.lib.frhip_stem_stats(L.code, L.p(L.x), L.p(L.wp), *L.geom, L.p(part), L.ops._s()), "frhip_stem_stats", partial=part)


def run_fwd(name, dt, keep_on_device=False):
    L = Launch(name, dt)
    hp, wp = sc.pooled_hw(L.case.h, L.case.w)
    pooled = L.mem.out((L.case.b, hp, wp, 64), L.dtype, "pooled")
    arg = L.mem.out((L.case.b, hp, wp, 64), torch.uint8, "argmax")
    out = L.done(L.lib.frhip_stem_fwd(L.code, L.p(L.x), L.p(L.wp), L.p(L.vec["scale"]), L.p(L.vec["shift"]), L.p(pooled), L.p(arg), *L.geom,
                                      L.ops._s()), "frhip_stem_fwd", pooled=pooled, arg=arg)
    return (out, pooled, arg) if keep_on_device else out


def run_reduce(name, dt, **own):
    L = Launch(name, dt, **own)
    dpool, arg = L.dpool(), L.arg()
    part = L.mem.out((L.blocks, 2, 64), torch.float32, "partial")
    v = L.vec
    return L.done(L.lib.frhip_stem_bwd_reduce(L.code, L.p(L.x), L.p(L.wp), L.p(dpool), L.p(arg), L.p(v["mean"]), L.p(v["invstd"]), L.p(v["scale"]),
                                              L.p(v["shift"]), *L.geom, L.p(part), L.ops._s()), "frhip_stem_bwd_reduce", partial=part)


def run_wgrad(name, dt, **own):
    L = Launch(name, dt, **own)
    dpool, arg, dw = L.dpool(), L.arg(), L.dw()
    slabs = L.mem.out((L.blocks, 2048), torch.float32, "slabs")
    v = L.vec
    return L.done(L.lib.frhip_stem_bwd_wgrad(L.code, L.p(L.x), L.p(L.wp), L.p(dpool), L.p(arg), L.p(v["ca"]), L.p(v["cb"]), L.p(v["cc"]),
                                             L.p(v["scale"]), L.p(v["shift"]), *L.geom, L.p(slabs), L.p(dw), L.ops._s()), "frhip_stem_bwd_wgrad", dw=dw)


def run_gram(name, dt):
    L = Launch(name, dt)
    part = L.mem.out((L.lib.frhip_stem_gram_blocks(*L.geom) + 1, sc.GRAM_OUT), torch.float32, "gram partial")
    gram = L.mem.out((L.lib.frhip_stem_gram_floats(),), torch.float32, "gram")
    return L.done(L.lib.frhip_stem_gram(L.code, L.p(L.x), *L.geom, L.p(part), L.p(gram), L.ops._s()), "frhip_stem_gram", gram=gram)


def run_wgrad_gram(name, dt, **own):
    """the Gram vector comes from the reference: frhip_stem_gram has its own test"""
    L = Launch(name, dt, **own)
    dpool, arg, pooled, dw = L.dpool(), L.arg(), L.pooled(), L.dw()
    gram = L.mem.put(L.ref["gram"], torch.float32, "gram")
    slabs = L.mem.out((L.blocks, 2048), torch.float32, "slabs")
    v = L.vec
    return L.done(L.lib.frhip_stem_bwd_wgrad_gram(L.code, L.p(L.x), L.p(L.wp), L.p(dpool), L.p(pooled), L.p(arg), L.p(gram), L.p(v["ca"]),
                                                  L.p(v["cb"]), L.p(v["cc"]), *L.geom, L.p(slabs), L.p(dw), L.ops._s()),
                  "frhip_stem_bwd_wgrad_gram", dw=dw)


def run_dx(name, dt, recompute, **own):
    """recompute: (cb, cc) given -- dy0 = ca d + cb y + cc; else the pair and x are NULL -- the eval-mode form dy0 = ca d"""
    L = Launch(name, dt, **own)
    dpool, arg, pooled = L.dpool(), L.arg(), L.pooled()
    dx = L.mem.out((L.case.b, 3, L.case.h, L.case.w), torch.float32, "dx")
    v = L.vec
    x, cb, cc = (L.p(L.x), L.p(v["cb"]), L.p(v["cc"])) if recompute else (None, None, None)
    return L.done(L.lib.frhip_stem_dx(L.code, x, L.p(L.wp), L.p(dpool), L.p(arg), L.p(pooled), L.p(v["ca"]), cb, cc, *L.geom, L.p(dx), L.ops._s()),
                  "frhip_stem_dx", dx=dx)


# ---------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name,dt", STATS)
def test_stats_partials_sum_to_the_exact_sums(name, dt):
    """frhip_stem_stats: exactly frhip_stem_blocks rows, each written, and their float64 sum is { sum y, sum y^2 } to the bit"""
    ref = sc.reference(name)
    part = twice(lambda: run_stats(name, dt), name)["partial"]
    assert part.shape == (sc.stem_blocks(sc.BY_NAME[name]), 2, 64) and not bool(torch.isnan(part).any()), "a partial row was not written"
    same(part.double().sum(0), torch.stack([ref["sum_y"], ref["sum_y2"]]), "{ sum y, sum y^2 }")


def check_forward(name, out):
    case, ref = sc.BY_NAME[name], sc.reference(name)
    pooled, arg = out["pooled"], out["arg"].long()
    # independent of the first-max rule: a byte names a tap of the window that lies in the image and holds the pooled value
    assert int(arg.max()) < 9, "an arg-max byte is not a tap index (0xFF: never written)"
    hh, ww = sc.argmax_pixel(arg)
    assert bool(((hh >= 0) & (hh < case.h) & (ww >= 0) & (ww < case.w)).all()), "an arg-max byte points outside the image"
    b, hp, wp, c = arg.shape
    at = ref["a"][torch.arange(b).view(b, 1, 1, 1), hh, ww, torch.arange(c).view(1, 1, 1, c)]
    same(pooled.double(), at, "the activation at the arg-max tap against the pooled value")
    same(pooled, ref["pooled"], "pooled")
    same(out["arg"], ref["arg"], "arg-max bytes against the first maximum in row-major tap order")


@pytest.mark.parametrize("name,dt", FULL)
def test_forward_pooled_values_and_first_max_bytes(name, dt):
    check_forward(name, twice(lambda: run_fwd(name, dt), name))


def check_reduce(name, part):
    assert part.shape == (sc.stem_blocks(sc.BY_NAME[name]), 2, 64) and not bool(torch.isnan(part).any()), "a partial row was not written"
    same(part.double().sum(0), sc.reference(name)["reduce"], "{ sum d, invstd (sum d y - mean sum d) }")


def check_dw(name, dw, what):
    same(dw.double(), sc.reference(name)["dw"] + sc.operands(name)["dw0"], what)


@pytest.mark.parametrize("name,dt,form", FORMS)
def test_backward_reduce_both_rows(name, dt, form):
    with backward_form(form, dt):
        check_reduce(name, twice(lambda: run_reduce(name, dt), name)["partial"])


@pytest.mark.parametrize("name,dt,form", FORMS)
def test_backward_weight_gradient_by_recompute(name, dt, form):
    with backward_form(form, dt):
        check_dw(name, twice(lambda: run_wgrad(name, dt), name)["dw"], "dw0 + sum dy col")


@pytest.mark.parametrize("name,dt", GRAM)
def test_gram_all_756_floats(name, dt):
    gram = twice(lambda: run_gram(name, dt), name)["gram"]
    assert gram.numel() == 756
    same(gram.double(), sc.reference(name)["gram"], "{ G, s }")


@pytest.mark.parametrize("name,dt", FULL)
def test_backward_weight_gradient_by_the_gram_form(name, dt):
    check_dw(name, twice(lambda: run_wgrad_gram(name, dt), name)["dw"], "dw0 + ca D + cb (W G) + cc s")


@pytest.mark.parametrize("recompute", [True, False], ids=["cb-cc", "null"])
@pytest.mark.parametrize("name,dt", FULL)
def test_image_gradient(name, dt, recompute):
    dx = twice(lambda: run_dx(name, dt, recompute), name)["dx"]
    same(dx.double(), sc.reference(name)["dx" if recompute else "dx_eval"], "dx")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("b,h,w,kp", sc.S2_CASES)
def test_image_gradient_of_the_stride_2_stem(b, h, w, kp, dt):
    """frhip_stem_dx_s2.  Its grid is capped at 65536 workgroups of 256 quads; the grid-stride trip beyond needs 16.8 M quads, which no
    small test reaches: that loop is not covered here."""
    ops, check, lib = _api()
    data, dtype = sc.s2_operands(b, h, w), sc.DTYPES[dt]
    assert torch.equal(data["dy0"].to(dtype).double(), data["dy0"])

    def run():
        mem = sc.Guarded()
        dy0 = mem.put(data["dy0"], dtype, "dy0")
        wp = mem.put(sc.packed_weights(data["w"], dtype, kp), dtype, "wp")
        dx = mem.out((b, 3, h, w), torch.float32, "dx")
        check(lib.frhip_stem_dx_s2(ops._DT[dtype], ops._p(dy0), ops._p(wp), kp, b, h, w, ops._p(dx), ops._s()), "frhip_stem_dx_s2")
        torch.cuda.synchronize()
        mem.check()
        return {"dx": dx.cpu()}

    same(twice(run, "s2")["dx"].double(), sc.stem_dx_s2(data["dy0"], data["w"], h, w), "dx, stride 2")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_device_forward_into_device_backward(dt):
    """2 x 9 x 57, two tile rows and two tile columns: the backward entry points on the arg-max bytes and the pooled map the device's own
    forward pass wrote, still on the device"""
    name = "2x9x57"
    out, pooled, arg = run_fwd(name, dt, keep_on_device=True)
    check_forward(name, out)
    own = dict(arg=arg, pooled=pooled)
    for form in (("gather",) if dt == "fp32" else ("scatter", "gather")):
        with backward_form(form, dt):
            check_reduce(name, run_reduce(name, dt, arg=arg)["partial"])
            check_dw(name, run_wgrad(name, dt, arg=arg)["dw"], "dw0 + sum dy col (%s)" % form)
    check_dw(name, run_wgrad_gram(name, dt, **own)["dw"], "dw0 + ca D + cb (W G) + cc s")
    same(run_dx(name, dt, True, **own)["dx"].double(), sc.reference(name)["dx"], "dx")
    same(run_dx(name, dt, False, **own)["dx"].double(), sc.reference(name)["dx_eval"], "dx, cb = cc = NULL")
