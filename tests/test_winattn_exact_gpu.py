"""The window-attention kernels (csrc/winattn.hip VALU, csrc/winattn_mfma.hip bf16 MFMA, the index arithmetic of csrc/winattn.h) on
the GPU at every window size, shift, map shape, window count and head count of tests/winattn_cases.py.

Exact regimes (see winattn_cases): a bias that makes the softmax one-hot turns attention into routing, so every implementation -- f32
(VALU), bf16-valu (MFMA switch off) and bf16-mfma -- must give out == v[sel] with torch.equal, and in the backward pass dv == the routed
dO, dq = dk = d(bias) = d(scale) = 0 (regime A, torch.equal; pre-filled accumulators keep their bits) or within LEAK = 1e-9 (regime B,
where the shift mask decides the selected key; S, where the head's scale does; R, where dv is a sum bf16 has to round and the column
sums must be those of the rounded values, within 128 LEAK).  A token routed to the wrong pixel, a one-token error in a mask region, a transposed
bias entry, a K slot that is not zero where the window has no key: each is an error of at least 1.  Every call runs twice with equal
bits and dqkv is the same bits in the plain, column-sum and q / v-bias forms.

Canaries: out, dqkv and the workspace carved from NaN-poisoned memory with guards on both sides (tests/stem_cases.Guarded over
tests/poison.py), the workspace at exactly heads * chunks * WA_PART floats; one float less is refused and nothing is written.

Numeric regime (random operands): the MFMA kernels through check_winattn of tests/test_bench_launches_gpu.py with its bounds, the VALU
kernels against the float64 attention with the tolerances of tests/test_swin_gpu.py::test_window_attention_kernel, on the same
geometries and with an all-zero q row and k row (the 1e-12 clamp)."""
import contextlib
import functools

import pytest
import torch

import winattn_cases as wc

pytestmark = pytest.mark.gpu

IMPLS = ("f32", "bf16-valu", "bf16-mfma")
IDS = [wc.case_id(c) for c in wc.CASES]
NUMERIC = IDS + ["zero-rows"]


def _api():
    from frhip import ops
    from frhip._abi import check, lib
    return ops, check, lib()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def implementation(impl):
    _, _, lib = _api()
    old = lib.frhip_set_winattn_mfma(1 if impl == "bf16-mfma" else 0)
    try:
        yield torch.float32 if impl == "f32" else torch.bfloat16
    finally:
        lib.frhip_set_winattn_mfma(old)


def bits(t):
    return t.contiguous().view(torch.uint8)


def twice(run, what):
    first, second = run(), run()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(first, second)):
        if isinstance(a, torch.Tensor):
            assert torch.equal(bits(a), bits(b)), "%s: result %d differs from run to run" % (what, i)
    return first


def same(got, want, what):
    got, want = got.float().cpu(), want.float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        g, w = got.double(), want.double()
        wrong = (g != w) | torch.isnan(g)
        raise AssertionError("%s: %d of %d elements differ, largest difference %r, first at %r: got %r, want %r" % (
            what, int(wrong.sum()), want.numel(), float((g - w).abs().nan_to_num(float("inf")).max()),
            tuple(wrong.nonzero()[0].tolist()), float(g[wrong][0]), float(w[wrong][0])))


def near(got, want, tol, what):
    err = (got.double().cpu() - want.double()).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), "%s: %d of %d elements further than %g, largest %r" % (
        what, int(bad.sum()), err.numel(), tol, float(err.nan_to_num(float("inf")).max()))


def small_ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randint(1, 9, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()).cuda()


def check_backward(o, regime, C, dqkv, dbias, dscale, what, dbias0=None, dscale0=None):
    """dqkv / d(bias) / d(scale) of one backward call against the closed form: regime A exactly, the others within their leak"""
    dv = o["dv_stored"] if dqkv.dtype == torch.bfloat16 else o["dv"]
    tol = wc.TOL[regime]
    zeros_qk = torch.zeros((dqkv.shape[0], 2 * C))
    db_want = torch.zeros_like(o["bias"]) if dbias0 is None else dbias0.cpu()
    ds_want = torch.zeros_like(o["scale"]) if dscale0 is None else dscale0.cpu()
    if regime == "A":
        same(dqkv[:, :2 * C], zeros_qk, what + ": dq, dk")
        same(dqkv[:, 2 * C:], dv, what + ": dv")
        if dbias0 is None:
            same(dbias, db_want, what + ": d(bias)")
            same(dscale, ds_want, what + ": d(scale)")
        else:                                                    # accumulators: the same bits as before the call
            assert torch.equal(bits(dbias.cpu()), bits(db_want)) and torch.equal(bits(dscale.cpu()), bits(ds_want)), what + ": accumulators"
    else:
        near(dqkv[:, :2 * C], zeros_qk, tol, what + ": dq, dk")
        near(dqkv[:, 2 * C:], dv, tol, what + ": dv")
        near(dbias, db_want, tol, what + ": d(bias)")
        near(dscale, ds_want, tol, what + ": d(scale)")


def run_exact(cid, regime, impl):
    ops, check, lib = _api()
    c, o = wc.BY_ID[cid], wc.operands(cid, regime)
    C, heads = 32 * c.heads, c.heads
    geom = (c.b, c.H, c.W, heads, c.ws, c.shift)
    what = "%s regime %s %s" % (cid, regime, impl)
    npix = c.b * c.H * c.W
    with implementation(impl) as dtype:
        qkv, dout = o["qkv"].to(dtype).cuda(), o["dout"].to(dtype).cuda()
        bias, scale = o["bias"].cuda(), o["scale"].cuda()
        out, = twice(lambda: (ops.winattn_fwd(qkv, bias, scale, *geom),), what + " forward")
        same(out, o["out"], what + ": out")
        dqkv, dbias, dscale = twice(lambda: ops.winattn_bwd(qkv, dout, bias, scale, *geom), what + " backward")
        check_backward(o, regime, C, dqkv, dbias, dscale, what + " backward")
        db0, ds0 = small_ints(bias.shape, 5), small_ints(scale.shape, 6)
        dqkv2, dbias2, dscale2 = twice(lambda: ops.winattn_bwd(qkv, dout, bias, scale, *geom, dbias=db0.clone(), dscale=ds0.clone()),
                                       what + " backward, accumulating")
        assert torch.equal(bits(dqkv2), bits(dqkv)), what + ": dqkv of the accumulate form"
        check_backward(o, regime, C, dqkv2, dbias2, dscale2, what + " backward, accumulating", db0, ds0)
        if impl != "bf16-mfma":
            return
        # ---- fused column sums of the stored dqkv, and the q / v thirds added into gradient accumulators
        sums = torch.cat([torch.zeros(2 * C), o["dv_colsum"]])
        tol = wc.TOL[regime] * npix                               # beyond regime A every stored element is within its leak
        dqkv3, dbias3, dscale3, colsum = twice(lambda: ops.winattn_bwd(qkv, dout, bias, scale, *geom, want_colsum=True), what + " column sums")
        assert torch.equal(bits(dqkv3), bits(dqkv)), what + ": dqkv of the column-sum form"
        check_backward(o, regime, C, dqkv3, dbias3, dscale3, what + " column sums")
        (same(colsum, sums, what + ": column sums") if regime == "A" else near(colsum, sums, tol, what + ": column sums"))
        gq0, gv0 = small_ints((C,), 7), small_ints((C,), 8)

        def into(want_q, want_v, through_ops):
            gq, gv = gq0.clone(), gv0.clone()
            grads = torch.empty_like(qkv)
            db, ds = db0.clone(), ds0.clone()
            if through_ops:
                grads, db, ds, flag = ops.winattn_bwd(qkv, dout, bias, scale, *geom, want_colsum=True, dbias=db, dscale=ds, qv_grads=(gq, gv))
                assert flag is True
            else:
                ws_ = ops.workspace(qkv.device)
                check(lib.frhip_winattn_bwd_qvbias(ops.dt_of(qkv), ops._p(qkv), ops._p(dout), ops._p(bias), ops._p(scale), ops._p(grads),
                                                   ops._p(db), ops._p(ds), ops._p(gq) if want_q else None, ops._p(gv) if want_v else None,
                                                   c.b, c.H, c.W, C, heads, c.ws, c.shift, ops._p(ws_), ws_.numel() * 4, ops._s()),
                      "frhip_winattn_bwd_qvbias")
            return grads, db, ds, gq, gv

        for want_q, want_v, through_ops in ((True, True, True), (True, False, False), (False, True, False)):
            form = what + " q / v bias gradients (%s, %s)" % ("q" if want_q else "NULL", "v" if want_v else "NULL")
            grads, db, ds, gq, gv = twice(lambda: into(want_q, want_v, through_ops), form)
            assert torch.equal(bits(grads), bits(dqkv)), form + ": dqkv"
            check_backward(o, regime, C, grads, db, ds, form, db0, ds0)
            # an accumulator passed as NULL keeps its bits; one passed holds its old integers + the sums (regime A: exactly)
            gv_want = gv0.cpu() + (o["dv_colsum"] if want_v else 0)
            for got, old, new, passed, third in ((gq, gq0, gq0.cpu(), want_q, "q"), (gv, gv0, gv_want, want_v, "v")):
                if not passed:
                    assert torch.equal(bits(got), bits(old)), form + ": %s accumulator was not passed" % third
                elif regime == "A":
                    same(got, new, form + ": %s accumulator" % third)
                else:
                    near(got, new, tol, form + ": %s accumulator" % third)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("cid", IDS)
def test_routing_is_exact(cid, impl):
    """regime A on every geometry, B (the mask decides) and R (sums bf16 rounds) on every shifted one, S (the scale decides) wherever
    there are two heads: forward, backward plain and accumulating, and on the MFMA kernels the column-sum form and the q / v
    bias-gradient form with both accumulators and with either one NULL"""
    c = wc.BY_ID[cid]
    for rule, rid in wc.RAGGED.items():
        if rid == cid and _cus() == wc.NOMINAL_CUS:
            assert wc.ragged(c, rule, _cus()), (rule, wc.chunking(c, rule, _cus()))
    for regime in wc.regimes_of(c):
        run_exact(cid, regime, impl)


# ---------------------------------------------------------------------------------------------------------------- canaries, workspace edge
WS_TEXT = "frhip_winattn_bwd: the workspace must hold %d partial-sum slots of %d floats"


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("cid", wc.CANARY)
def test_guarded_buffers_and_the_exact_workspace(cid, impl):
    from stem_cases import Guarded
    import poison
    ops, check, lib = _api()
    c = wc.BY_ID[cid]
    regime = "B" if c.shift else "A"
    o = wc.operands(cid, regime)
    C, heads, npix = 32 * c.heads, c.heads, c.b * c.H * c.W
    geom = (c.b, c.H, c.W, C, heads, c.ws, c.shift)
    chunks = wc.chunking(c, "bwd-mfma" if impl == "bf16-mfma" else "bwd-valu", _cus())[0]
    floats = heads * chunks * wc.WA_PART
    with implementation(impl) as dtype:
        code = ops._DT[dtype]
        mem = Guarded()
        qkv, dout = mem.put(o["qkv"], dtype, "qkv"), mem.put(o["dout"], dtype, "dout")
        bias, scale = mem.put(o["bias"], torch.float32, "bias"), mem.put(o["scale"], torch.float32, "scale")
        want_out = ops.winattn_fwd(qkv, bias, scale, c.b, c.H, c.W, heads, c.ws, c.shift)
        want = ops.winattn_bwd(qkv, dout, bias, scale, c.b, c.H, c.W, heads, c.ws, c.shift, want_colsum=impl == "bf16-mfma")
        out = mem.out((npix, C), dtype, "out")
        check(lib.frhip_winattn_fwd(code, ops._p(qkv), ops._p(bias), ops._p(scale), ops._p(out), *geom, ops._s()), "frhip_winattn_fwd")
        torch.cuda.synchronize()
        mem.check()
        assert torch.equal(bits(out), bits(want_out))
        same(out, o["out"], cid + ": out")

        def backward(ws_floats, colsum):
            dqkv = mem.out((npix, 3 * C), dtype, "dqkv")
            dbias, dscale = mem.put(torch.zeros_like(o["bias"]), torch.float32, "dbias"), mem.put(torch.zeros_like(o["scale"]), torch.float32, "dscale")
            work = mem.out((ws_floats,), torch.float32, "workspace")
            args = (code, ops._p(qkv), ops._p(dout), ops._p(bias), ops._p(scale), ops._p(dqkv), ops._p(dbias), ops._p(dscale))
            tail = geom + (ops._p(work), ws_floats * 4, ops._s())
            cs = None
            if colsum:
                cs = mem.put(torch.zeros(3 * C), torch.float32, "colsum")
                rc = lib.frhip_winattn_bwd_colsum(*args, ops._p(cs), *tail)
            else:
                rc = lib.frhip_winattn_bwd(*args, *tail)
            torch.cuda.synchronize()
            mem.check()
            return rc, dqkv, dbias, dscale, work, cs

        for colsum in ((False, True) if impl == "bf16-mfma" else (False,)):
            rc, dqkv, dbias, dscale, work, cs = backward(floats, colsum)
            check(rc, "frhip_winattn_bwd")
            for got, ref in zip((dqkv, dbias, dscale), want):
                assert torch.equal(bits(got), bits(ref)), (cid, impl, colsum)
            if colsum:
                assert torch.equal(bits(cs), bits(want[3]))
            # one float less: refused before anything is launched
            rc, dqkv, dbias, dscale, work, cs = backward(floats - 1, colsum)
            assert rc == -1 and lib.frhip_last_error() == (WS_TEXT % (heads * chunks, wc.WA_PART)).encode()
            assert poison.holds(dqkv, float("nan")) and poison.holds(work, float("nan"))
            assert not bool(dbias.any()) and not bool(dscale.any()) and (cs is None or not bool(cs.any()))


# ---------------------------------------------------------------------------------------------------------------- numeric regime
def _numeric_case(name):
    return wc.ZERO_ROW_GEOM if name == "zero-rows" else wc.BY_ID[name]


@pytest.mark.parametrize("name", NUMERIC)
def test_mfma_kernels_against_float64_on_random_operands(name, monkeypatch):
    """check_winattn of tests/test_bench_launches_gpu.py (float64 with the kernels' bf16 roundings, per-element bounds; the accumulate
    form, the column sums and the q / v bias gradients included) with its bounds as they are, on every geometry of the table"""
    import test_bench_launches_gpu as tb
    c = _numeric_case(name)
    C = 32 * c.heads
    if name == "zero-rows":
        inputs = tb._attn_inputs

        def with_zero_rows(*args):
            qkv, bias, scale, dout = inputs(*args)
            qkv[wc.ZERO_Q_PIXEL, :32] = 0
            qkv[wc.ZERO_K_PIXEL, C + 32:C + 64] = 0
            return qkv, bias, scale, dout
        monkeypatch.setattr(tb, "_attn_inputs", with_zero_rows)
    tb.check_winattn(c.b, c.H, c.W, C, c.heads, c.ws, c.shift)


@functools.lru_cache(maxsize=None)
def numeric_reference(name):
    c = _numeric_case(name)
    qkv, bias, scale, dout = wc.numeric_operands(c, zero_rows=name == "zero-rows")
    pix, region = wc.index_maps(wc.case_id(c))
    out, dqkv, dbias, dscale, _, _ = wc.attention64_grads(qkv, dout, bias, scale, pix, region, c.heads)
    return (qkv, bias, scale, dout), (out, dqkv, dbias, dscale)


def allclose(got, ref, rtol, atol, what):
    err = (got.double().cpu() - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())
    assert not bool(bad.any()), "%s: %d of %d elements outside rtol %g atol %g, largest error %r" % (
        what, int(bad.sum()), err.numel(), rtol, atol, float(err.nan_to_num(float("inf")).max()))


@pytest.mark.parametrize("impl", IMPLS[:2])
@pytest.mark.parametrize("name", NUMERIC)
def test_valu_kernels_against_float64_on_random_operands(name, impl):
    """the fp32-arithmetic kernels in fp32 and bf16 against the float64 attention without operand roundings, shifted and small windows
    included, with the tolerances of tests/test_swin_gpu.py::test_window_attention_kernel"""
    ops, _, _ = _api()
    c = _numeric_case(name)
    C = 32 * c.heads
    (qkv, bias, scale, dout), (out_ref, dqkv_ref, dbias_ref, dscale_ref) = numeric_reference(name)
    geom = (c.b, c.H, c.W, c.heads, c.ws, c.shift)
    what = "%s %s" % (name, impl)
    with implementation(impl) as dtype:
        out = ops.winattn_fwd(qkv.to(dtype).cuda(), bias.cuda(), scale.cuda(), *geom)
        dqkv, dbias, dscale = ops.winattn_bwd(qkv.to(dtype).cuda(), dout.to(dtype).cuda(), bias.cuda(), scale.cuda(), *geom)
    rtol, atol = (2e-4, 2e-5) if dtype == torch.float32 else (3e-2, 3e-2)
    allclose(out, out_ref, rtol, atol, what + ": out")
    allclose(dqkv, dqkv_ref, rtol, atol * max(float(dqkv_ref.abs().max()), 1.0), what + ": dqkv")
    if name == "zero-rows":
        # the two clamped rows carry gradients of order 1e12 and would set the absolute tolerance of everything else: the rest again,
        # with the tolerance its own largest gradient gives
        rest = torch.ones_like(dqkv_ref, dtype=torch.bool)
        rest[wc.ZERO_Q_PIXEL, :32] = False
        rest[wc.ZERO_K_PIXEL, C + 32:C + 64] = False
        allclose(dqkv.cpu()[rest], dqkv_ref[rest], rtol, atol * max(float(dqkv_ref[rest].abs().max()), 1.0), what + ": dqkv off the zero rows")
    allclose(dbias, dbias_ref, 2e-3, 2e-3 * float(dbias_ref.abs().max()), what + ": d(bias)")
    allclose(dscale, dscale_ref, 2e-3, 2e-3 * float(dscale_ref.abs().max()), what + ": d(scale)")
