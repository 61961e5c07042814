"""The window-attention case table (tests/winattn_cases.py) without a GPU: that it holds every geometry the branches of
csrc/winattn.hip / winattn_mfma.hip / winattn.h need, what each case covers (tile count, idle waves, xcd_remap remainder, mask regions,
ragged chunks), that the closed-form expectations of the two exact regimes are what a float64 attention with autograd gives on the same
operands, and the host-side refusals of the four entry points (return code and the whole frhip_last_error text)."""
import pytest
import torch

import winattn_cases as wc

IDS = [wc.case_id(c) for c in wc.CASES]
SHIFTED_IDS = [wc.case_id(c) for c in wc.SHIFTED]
EXACT = [(cid, regime) for cid in IDS for regime in wc.regimes_of(wc.BY_ID[cid])]


def test_table_holds_every_required_geometry():
    need = []
    for ws in range(1, 8):
        need.append((2 * ws, 2 * ws, ws, 0))
    for ws in range(2, 8):
        for shift in {1, ws // 2, ws - 1}:
            need.append((2 * ws, 2 * ws, ws, shift))
    have = {(c.H, c.W, c.ws, c.shift) for c in wc.CASES}
    assert not [g for g in need if g not in have]
    shifted = lambda pred: [c for c in wc.CASES if c.shift and pred(c)]
    assert shifted(lambda c: (c.H, c.W) == (2 * c.ws, 3 * c.ws)) and shifted(lambda c: (c.H, c.W) == (3 * c.ws, c.ws))
    assert shifted(lambda c: c.H == c.W == c.ws and c.b == 1)
    assert shifted(lambda c: c.H == c.ws and c.W == 2 * c.ws)
    for ws in (7, 5):
        assert {1, 2, 3, 4, 5, 9} <= {wc.nwin_of(c) for c in wc.CASES if c.ws == ws}
    assert {1, 3, 5, 16} <= {c.heads for c in wc.CASES}
    assert {1, 2, 3} <= {c.b for c in wc.CASES}
    assert all(c.why for c in wc.CASES) and len(set(IDS)) == len(IDS)
    for c in wc.CASES:                                           # what frhip_winattn_* accepts, and tensors of a few MB at the most
        assert 1 <= c.ws <= 7 and c.H % c.ws == 0 and c.W % c.ws == 0 and 0 <= c.shift < c.ws
        assert c.b * c.H * c.W * 3 * 32 * c.heads * 4 <= 4 << 20


def test_every_tile_count_is_launched():
    """wm_fwd_kernel<NT> / wm_bwd_kernel<NT> for NT 1 .. 4, shifted and not; ws 5 alone gives NT 2, ws 4 fills its one tile"""
    nts = {ws: (ws * ws + 15) // 16 for ws in range(1, 8)}
    assert nts == {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 3, 7: 4}
    for c in wc.CASES:
        assert wc.nt_of(c) == nts[c.ws]
    for shifted in (False, True):
        assert {wc.nt_of(c) for c in wc.CASES if bool(c.shift) == shifted} == {1, 2, 3, 4}
    assert any(c.ws == 4 and wc.n_of(c) == 16 * wc.nt_of(c) for c in wc.CASES)            # no padded key at all
    assert any(c.ws == 1 for c in wc.CASES)


IDLE = {1: 3, 2: 2, 3: 1, 4: 0, 5: 3, 9: 3}           # windows -> idle waves of the last workgroup (chunks of four windows)


def test_idle_waves_and_grid_remainders():
    for ws in (7, 5):
        for nwin, idle in IDLE.items():
            cs = [c for c in wc.CASES if c.ws == ws and wc.nwin_of(c) == nwin and not c.shift]
            assert cs, (ws, nwin)
            for c in cs:
                for rule in wc.RULES:
                    chunks, wpb, last = wc.chunking(c, rule)
                    assert wpb == 4 and chunks == -(-nwin // 4) and 4 - min(4, last) == idle == wc.idle_waves(c, rule)
    # heads * chunks mod 8: the remainder branch of xcd_remap (r != 0) with 1, 2, 3, 5, 6 workgroups over; r == 0 with 16 heads
    rem = {}
    for c in wc.CASES:
        for rule in ("fwd-mfma", "bwd-mfma"):
            rem.setdefault(c.heads * wc.chunking(c, rule)[0] % 8, wc.case_id(c))
    assert {0, 1, 2, 3, 5, 6} <= set(rem), rem
    for heads, want in ((1, 1), (3, 3), (5, 5)):
        c = wc.BY_ID["b1-14x14-h%d-ws7-s3" % heads]
        assert wc.chunking(c, "fwd-mfma")[0] == wc.chunking(c, "bwd-mfma")[0] == 1 and c.heads % 8 == want
    assert (16 * wc.chunking(wc.BY_ID["b1-10x10-h16-ws5-s2"], "bwd-mfma")[0]) % 8 == 0


def test_xcd_remap_is_a_permutation_of_every_grid_of_the_table():
    """common.h xcd_remap restated: the (head, chunk) decode behind it must reach every pair once, remainder or not"""
    def remap(bid, nwg):
        q, r, xcd, k = nwg >> 3, nwg & 7, bid & 7, bid >> 3
        return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + k
    for nwg in sorted({c.heads * wc.chunking(c, rule)[0] for c in wc.CASES for rule in ("fwd-mfma", "bwd-mfma")}):
        assert sorted(remap(b, nwg) for b in range(nwg)) == list(range(nwg)), nwg


def test_mask_regions_per_case():
    for c in wc.CASES:
        regions = wc.regions_of(c)
        rows = {1, 2} if c.H == c.ws else {0, 1, 2}
        cols = {1, 2} if c.W == c.ws else {0, 1, 2}
        want = tuple(sorted(3 * r + q for r in rows for q in cols)) if c.shift else (0,)
        assert regions == want, (wc.case_id(c), regions)
    assert wc.regions_of(wc.BY_ID["b1-7x7-h2-ws7-s3"]) == (4, 5, 7, 8)
    assert wc.regions_of(wc.BY_ID["b1-7x14-h2-ws7-s3"]) == (3, 4, 5, 6, 7, 8)
    assert wc.regions_of(wc.BY_ID["b1-21x7-h2-ws7-s3"]) == (1, 2, 4, 5, 7, 8)
    assert wc.regions_of(wc.BY_ID["b1-14x14-h2-ws7-s6"]) == tuple(range(9))


def test_ragged_chunk_cases():
    """one case per chunk rule with several windows per wave and a shorter last chunk (at 256 CUs)"""
    want = {"fwd-mfma": (898, 5, 4), "bwd-mfma": (218, 5, 4), "bwd-valu": (54, 6, 5)}
    for rule, cid in wc.RAGGED.items():
        c = wc.BY_ID[cid]
        assert wc.chunking(c, rule) == want[rule] and wc.ragged(c, rule), (rule, wc.chunking(c, rule))
    assert wc.chunking(wc.BY_ID[wc.RAGGED["fwd-mfma"]], "bwd-valu") == (898, 5, 4)          # heads 1: the same 1024-workgroup target
    for cid in wc.CANARY:
        assert cid in wc.BY_ID


@pytest.mark.parametrize("cid", IDS)
def test_permutations(cid):
    c = wc.BY_ID[cid]
    n = wc.n_of(c)
    pi, rho = wc.permutations(cid)
    ident = torch.arange(n)
    for h in range(c.heads):
        assert sorted(pi[h].tolist()) == list(range(n))
        assert n == 1 or not torch.equal(pi[h], ident)
        if rho is not None:
            assert sorted(rho[h].tolist()) == list(range(n)) and not bool((rho[h] == pi[h]).any())
    if len(wc.affine_perms(n)) >= c.heads:
        assert len({tuple(p.tolist()) for p in pi}) == c.heads
    if c.shift:
        o = wc.operands(cid, "B")
        by_mask = o["sel"] != o["pi"][None]
        assert bool(by_mask.any()) and not bool(by_mask.all())
        for h in range(c.heads):                                   # every head has queries decided each way
            assert bool(by_mask[:, h].any()) and not bool(by_mask[:, h].all()), (cid, h)
        # a query the mask decides really has its pi key in another region and its rho key in its own
        reg = o["region"]
        for h in range(c.heads):
            other = reg[:, o["pi"][h]] != reg
            same = reg[:, o["rho"][h]] == reg
            assert torch.equal(by_mask[:, h], other & same)


@pytest.mark.parametrize("cid,regime", EXACT, ids=["%s-%s" % e for e in EXACT])
def test_closed_forms_against_float64_attention(cid, regime):
    """the one-hot claims (arg-max, logit gaps, leak) and the expected out / dv / zero gradients against float64 autograd"""
    c = wc.BY_ID[cid]
    o = wc.operands(cid, regime)
    n, C = wc.n_of(c), 32 * c.heads
    qkv, dout = o["qkv"], o["dout"]
    # operand claims: bf16 holds every element; v, dO non-zero integers within their ranges; sums within the exact ranges
    assert torch.equal(qkv.bfloat16().float(), qkv) and torch.equal(dout.bfloat16().float(), dout)
    v = qkv[:, 2 * C:]
    assert torch.equal(v, v.round()) and 1 <= float(v.abs().min()) and float(v.abs().max()) <= wc.V_MAX
    assert torch.equal(dout, dout.round()) and 1 <= float(dout.abs().min())
    if regime == "R":
        assert set(dout.abs().unique().tolist()) == {1.0, float(wc.DO_BIG)}
        changed = o["dv_stored"] != o["dv"]                       # sums bf16 does not hold, and column sums that show it
        assert int(changed.sum()) >= 8 and float((o["dv_stored"] - o["dv"]).abs()[changed].min()) >= 1
        assert int((o["dv_colsum"] != o["dv"].sum(0)).sum()) >= 4
    else:
        assert float(dout.abs().max()) <= wc.DO_MAX and wc.DO_MAX * n < 256 and float(o["dv"].abs().max()) < 256
        assert torch.equal(o["dv_stored"], o["dv"])
    assert float(o["out"].abs().max()) <= wc.V_MAX
    assert float(dout.abs().sum(0).max()) + 8 < 2 ** 24           # the fp32 column sums, on top of accumulators of magnitude <= 8
    assert torch.equal(o["dv_colsum"], o["dv_stored"].sum(0))
    if regime == "S":
        assert o["scale"].tolist() == [wc.SCALES_S[h % 2] for h in range(c.heads)]
        for h in range(c.heads):                                  # the scale decides: even heads keep pi, odd heads take rho ...
            mine = o["rho"][h] if h % 2 else o["pi"][h]
            assert bool((o["sel"][:, h] == mine[None]).any())
        # ... and with head 0's scale an odd head would select other keys
        rows = torch.arange(n)
        cos = ((o["rho"][1] % 32)[:, None] == (rows % 32)[None, :]).double()
        masked = (o["region"][:, :, None] != o["region"][:, None, :]).double()
        other = (wc.SCALES_S[0] * cos[None] + o["bias"][1].double()[None] - 100.0 * masked).argmax(-1)
        assert int((other != o["sel"][:, 1]).sum()) >= 1
    else:
        assert float(o["scale"].max()) <= 4 and set(o["scale"].tolist()) <= set(wc.SCALES)
    out, dqkv, dbias, dscale, P, logit = wc.attention64_grads(qkv, dout, o["bias"], o["scale"], o["pix"], o["region"], c.heads)
    sel = o["sel"]                                               # [nwin, heads, n]
    assert torch.equal(P.argmax(-1), sel)
    top = torch.gather(logit, 3, sel[..., None])
    rest = logit.scatter(3, sel[..., None], float("-inf"))
    if n > 1:
        gap = top.squeeze(-1) - rest.amax(-1)
        if regime == "A":
            assert float(gap.min()) >= wc.GAP_A
        else:
            assert float(gap.min()) >= wc.GAP_B
            third = torch.sort(rest, -1, descending=True)[0][..., 1] if n > 2 else None
            if third is not None:                                # the -300 tier: exactly 0 in fp32
                assert float((top.squeeze(-1) - third).min()) > wc.EXP_ZERO
    # the leaked mass: at most n e^-gap (e^-32 < 2^-46, e^-192 < 2^-276; float64 holds the latter, fp32 has exp(x) == 0 below -104)
    assert float(torch.tensor(-wc.EXP_ZERO).exp()) == 0.0 and wc.GAP_A > wc.EXP_ZERO
    leak = 1 - torch.gather(P, 3, sel[..., None])
    assert float(leak.max()) <= n * 2.0 ** (-276 if regime == "A" else -46)
    # closed forms: within the leak times the largest |dP| = 32 * 8 * 2 and the 49 keys
    tol = 2.0 ** -250 if regime == "A" else wc.TOL[regime]
    assert float((out - o["out"].double()).abs().max()) <= tol
    assert float((dqkv[:, 2 * C:] - o["dv"].double()).abs().max()) <= tol
    assert float(dqkv[:, :2 * C].abs().max()) <= tol and float(dbias.abs().max()) <= tol and float(dscale.abs().max()) <= tol
    # out rounds to v[sel] in fp32 and bf16: the leak is below half an fp32 step of the smallest |v| = 1
    assert torch.equal(out.float(), o["out"])
    assert torch.equal(dout.sum(0), o["dv"].sum(0))               # every query selects one key: dv only moves dO around
    if regime == "A":                                            # dv is a permutation of dO inside every window
        inv = torch.argsort(o["pi"], 1)
        G = dout[o["pix"].reshape(-1)].view(-1, n, c.heads, 32)
        want = torch.stack([G[:, inv[h], h] for h in range(c.heads)], 2)
        assert torch.equal(o["dv"][o["pix"].reshape(-1)].view(-1, n, c.heads, 32), want)


def test_numeric_zero_rows_reach_the_clamp():
    c = wc.ZERO_ROW_GEOM
    qkv, bias, scale, dout = wc.numeric_operands(c, zero_rows=True)
    C = 32 * c.heads
    assert float(qkv[wc.ZERO_Q_PIXEL, :32].abs().max()) == 0 and float(qkv[wc.ZERO_K_PIXEL, C + 32:C + 64].abs().max()) == 0
    pix, region = wc.index_maps(wc.case_id(c))
    out, dqkv, dbias, dscale, P, _ = wc.attention64_grads(qkv, dout, bias, scale, pix, region, c.heads)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
    assert float(dqkv[wc.ZERO_Q_PIXEL, :32].abs().max()) > 1e6             # d(q) = d(q^) / 1e-12 at the clamp


# ---------------------------------------------------------------------------------------------------------------- host refusals
SHAPE_TEXT = "%s: needs ws <= 7 dividing h and w, 0 <= shift < ws, head dim 32 (c=%d heads=%d h=%d w=%d ws=%d shift=%d)"
COLSUM_TEXT = "%s: only the bf16 MFMA kernels produce the column sums (frhip_set_winattn_mfma)"
# (h, w, c, heads, ws, shift)
BAD_SHAPES = {"ws 0": (14, 14, 64, 2, 0, 0), "ws 8": (16, 16, 64, 2, 8, 0), "h % ws": (15, 14, 64, 2, 7, 0), "w % ws": (14, 15, 64, 2, 7, 0),
              "shift == ws": (14, 14, 64, 2, 7, 7), "shift -1": (14, 14, 64, 2, 7, -1), "c != 32 heads": (14, 14, 96, 2, 7, 0)}


def _call(lib, name, dtype, h, w, c, heads, ws, shift):
    """the entry point with NULL operands: a refusal must come before any of them is read"""
    geom = (1, h, w, c, heads, ws, shift)
    if name == "frhip_winattn_fwd":
        return lib.frhip_winattn_fwd(dtype, None, None, None, None, *geom, None)
    if name == "frhip_winattn_bwd":
        return lib.frhip_winattn_bwd(dtype, None, None, None, None, None, None, None, *geom, None, 0, None)
    if name == "frhip_winattn_bwd_colsum":
        return lib.frhip_winattn_bwd_colsum(dtype, None, None, None, None, None, None, None, None, *geom, None, 0, None)
    return lib.frhip_winattn_bwd_qvbias(dtype, None, None, None, None, None, None, None, None, None, *geom, None, 0, None)


ENTRIES = ("frhip_winattn_fwd", "frhip_winattn_bwd", "frhip_winattn_bwd_colsum", "frhip_winattn_bwd_qvbias")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from frhip import _abi
    return _abi.lib()


@pytest.mark.parametrize("what", sorted(BAD_SHAPES))
@pytest.mark.parametrize("name", ENTRIES)
def test_bad_window_geometry_is_refused(lib, name, what):
    shape = BAD_SHAPES[what]
    for dtype in (0, 1):
        assert _call(lib, name, dtype, *shape) == -1
        h, w, c, heads, ws, shift = shape
        assert lib.frhip_last_error() == (SHAPE_TEXT % (name, c, heads, h, w, ws, shift)).encode()


@pytest.mark.parametrize("name", ["frhip_winattn_bwd_colsum", "frhip_winattn_bwd_qvbias"])
def test_column_sums_are_refused_without_the_mfma_kernels(lib, name):
    good = (14, 14, 64, 2, 7, 3)
    assert lib.frhip_set_winattn_mfma(-1) == 1
    assert _call(lib, name, 1, *good) == -1                       # fp32
    assert lib.frhip_last_error() == (COLSUM_TEXT % name).encode()
    old = lib.frhip_set_winattn_mfma(0)
    try:
        assert _call(lib, name, 0, *good) == -1                   # bf16 with the MFMA switch off
        assert lib.frhip_last_error() == (COLSUM_TEXT % name).encode()
    finally:
        lib.frhip_set_winattn_mfma(old)
    assert lib.frhip_set_winattn_mfma(-1) == 1
