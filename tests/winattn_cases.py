"""Exact-routing cases of the window attention (csrc/winattn.hip, csrc/winattn_mfma.hip, the index arithmetic of csrc/winattn.h): one
minimal geometry per branch, and operands whose expected result is known in closed form.  Shared by tests/test_winattn_cases_cpu.py
(the table, the closed forms against a float64 attention with autograd; no GPU) and tests/test_winattn_exact_gpu.py.

Attention has a softmax, so integer operands alone do not make it exact; a bias that makes the softmax one-hot does.  Four regimes:

  A, permutation.  Per head h a permutation pi_h of the n tokens; bias[h][i][pi_h(i)] = 0 and BIAS_OFF = -300 everywhere else; scale[h]
     cycles through SCALES (at most 4), so |cos * scale| <= 4.  The target's logit is at least -4 - 100 (it may be masked), every other
     logit at most 4 - 300: a gap of at least GAP_A = 192.  exp(x) is exactly 0 in fp32 below -104, so P is exactly one-hot in every
     implementation, whatever the mask says: out[i] = v[pi(i)], dv[j] = dO[pi^-1(j)], and dq = dk = d(bias) = d(scale) = 0, all compared
     with torch.equal.  v and dO are small non-zero integers (|v| <= 8, |dO| <= 2): every sum bf16 stores stays below 256, every fp32
     column sum below 2^24.
  B, the mask decides (shifted cases).  A second permutation rho_h with rho_h(i) != pi_h(i); bias 0 at pi, BIAS_RHO = -40 at rho,
     BIAS_OFF elsewhere.  The selected key sel(w, i) is rho(i) when pi(i) lies in another mask region than i and rho(i) in the same one,
     and pi(i) otherwise.  The winner leads the runner-up by at least GAP_B = 40 - 2 * 4 = 32 and the -300 tier by more than 104, so the
     probability mass that leaks is at most n e^-32 < 2^-25: fp32 accumulation (and the bf16 rounding of the output) absorbs it in the
     forward pass, out == v[sel] exactly; in the backward pass it is of order 1e-12, and any misrouting is an error of at least 1, so
     LEAK = 1e-9 bounds dq, dk, d(bias), d(scale) and dv - sum_{i: sel(i) = j} dO_i.
  R, rounding (shifted cases): regime B with dO from {+-1, +-256}.  Where two queries select one key, dv is 257 or a like sum that bf16
     does not hold: the stored dv is its round-to-nearest-even, and the fused column sums are those of the STORED values.  The leak
     grows with |dO|: LEAK * 128.
  S, the scale decides (heads >= 2): q and k are unit vectors along one coordinate, k_j along j mod 32 and q_i along rho(i) mod 32,
     so every cosine is exactly 0 or 1 and cos(i, rho(i)) = 1; bias 0 at pi, BIAS_S = -48 at rho, BIAS_OFF elsewhere; scale[h] is 16
     on even heads (pi leads rho by 32) and 96 on odd heads (rho leads pi by 48).  All logits are small integers, the selected key is
     their arg-max (the mask included), gaps as in B.  A head that read another head's scale routes to the wrong key.

The pixel and region maps come from tests/ref64.window_index (held to the rolled partition with the slice mask by
tests/test_ref64_cpu.py).  The numeric regime (random operands) runs on the same geometries plus ZERO_ROW_GEOM."""
import collections
import functools
import math
import zlib

import torch

from ref64 import window_index

WA_PART = 49 * 49 + 1 + 3 * 32                  # floats per partial-sum slot (csrc/winattn.h)
NOMINAL_CUS = 256                               # MI355X; the GPU test recomputes the chunk rules from the device's own count
BIAS_OFF, BIAS_RHO, BIAS_S = -300.0, -40.0, -48.0
SCALES = (0.5, 1.0, 2.0, 4.0)
SCALES_S = (16.0, 96.0)
DO_BIG = 256                                    # regime R: 256 + 1 is not a bf16 number
TOL = {"A": 0.0, "B": 1e-9, "R": 128e-9, "S": 1e-9}
GAP_A, GAP_B, EXP_ZERO = 192.0, 32.0, 104.0     # logit gaps of the two regimes; fp32 exp(x) == 0 for x < -104
LEAK = 1e-9
V_MAX, DO_MAX = 8, 2

Case = collections.namedtuple("Case", "b H W heads ws shift why")


def case_id(c):
    return "b%d-%dx%d-h%d-ws%d-s%d" % (c.b, c.H, c.W, c.heads, c.ws, c.shift)


def n_of(c):
    return c.ws * c.ws


def nwin_of(c):
    return c.b * (c.H // c.ws) * (c.W // c.ws)


def nt_of(c):
    """16-token tiles per window: the template argument of wm_fwd_kernel / wm_bwd_kernel"""
    return (n_of(c) + 15) // 16


def wm_chunks(nwin, heads, target_wgs):
    """csrc/winattn_mfma.hip wm_chunks and the same rule in frhip_winattn_bwd: (chunks, windows per chunk)"""
    chunks = -(-target_wgs // heads)
    wpb = max(4, -(-nwin // chunks))
    return -(-nwin // wpb), wpb


RULES = {"fwd-mfma": lambda cus: 4 * cus, "bwd-mfma": lambda cus: cus, "bwd-valu": lambda cus: 1024}


def chunking(c, rule, cus=NOMINAL_CUS):
    """-> (chunks, windows per chunk, windows of the last chunk) of one of the three chunk rules"""
    chunks, wpb = wm_chunks(nwin_of(c), c.heads, RULES[rule](cus))
    return chunks, wpb, nwin_of(c) - (chunks - 1) * wpb


def ragged(c, rule, cus=NOMINAL_CUS):
    """several windows per wave AND a last chunk shorter than the others"""
    chunks, wpb, last = chunking(c, rule, cus)
    return chunks > 1 and wpb > 4 and last < wpb


def idle_waves(c, rule="bwd-mfma", cus=NOMINAL_CUS):
    """waves of the last workgroup that never enter the window loop but take part in the folds"""
    return 4 - min(4, chunking(c, rule, cus)[2])


def regions_of(c):
    return tuple(sorted(set(window_index(c.b, c.H, c.W, c.ws, c.shift, device="cpu")[1].reshape(-1).tolist())))


# ---------------------------------------------------------------------------------------------------------------- the table
def _table():
    t = collections.OrderedDict()

    def add(b, H, W, heads, ws, shift, why):
        key = (b, H, W, heads, ws, shift)
        t[key] = t[key] + "; " + why if key in t else why

    nt_why = {1: "one key, 63 idle lanes (NT 1)", 2: "n = 4 (NT 1)", 3: "n = 9 (NT 1)", 4: "n = 16: one full tile, no padded key (NT 1)",
              5: "n = 25: wm_fwd_kernel<2> / wm_bwd_kernel<2> (NT 2)", 6: "n = 36 (NT 3, odd: the zero K-slot tile)", 7: "n = 49 (NT 4)"}
    for ws in range(1, 8):
        add(1, 2 * ws, 2 * ws, 2, ws, 0, "ws %d unshifted, four windows: %s" % (ws, nt_why[ws]))
    for ws in range(2, 8):
        for shift in sorted({1, ws // 2, ws - 1}):
            add(1, 2 * ws, 2 * ws, 2, ws, shift, "ws %d shift %d: all nine regions" % (ws, shift))
    for ws, shift in ((7, 3), (5, 2), (3, 1)):
        add(1, 2 * ws, 3 * ws, 2, ws, shift, "H != W: wide map")
        add(1, 3 * ws, ws, 2, ws, shift, "H != W: tall map one window wide (no column region 0)")
    for ws, shift in ((7, 3), (5, 2), (4, 1), (2, 1)):
        add(1, ws, ws, 2, ws, shift, "H == W == ws shifted: one window, regions 1 and 2 only on both axes")
    for ws, shift in ((7, 3), (5, 4)):
        add(1, ws, 2 * ws, 2, ws, shift, "H == ws, W == 2 ws shifted: row regions 1 and 2 only")
    for ws in (7, 5):
        add(1, ws, ws, 2, ws, 0, "nwin 1: three waves idle in the folds")
        add(2, ws, ws, 2, ws, 0, "nwin 2, b 2: two waves idle")
        add(3, ws, ws, 2, ws, 0, "nwin 3, b 3: one wave idle")
        add(1, 2 * ws, 2 * ws, 2, ws, 0, "nwin 4: every wave one window")
        add(5, ws, ws, 2, ws, 0, "nwin 5: two chunks, the last with one window")
        add(1, 3 * ws, 3 * ws, 2, ws, 0, "nwin 9: three chunks")
    for heads in (1, 3, 5):
        add(1, 14, 14, heads, 7, 3, "heads %d: remainder branch of xcd_remap" % heads)
    add(1, 10, 10, 16, 5, 2, "heads 16 (grid a multiple of 8) at NT 2")
    add(2, 10, 10, 3, 5, 2, "b 2, heads 3 at NT 2")
    # ragged multi-window chunks (at 256 CUs): 4489 windows in chunks of 5 leave 4; 1089 in chunks of 5 leave 4; 323 in chunks of 6 leave 5
    add(1, 67, 67, 1, 1, 0, "ragged forward MFMA chunks (ceil(4 CUs / heads)) and ragged backward VALU chunks (ceil(1024 / heads)), heads 1")
    add(1, 66, 66, 1, 2, 1, "ragged backward MFMA chunks (ceil(CUs / heads))")
    add(1, 17, 19, 16, 1, 0, "ragged backward VALU chunks (ceil(1024 / heads)) with heads 16")
    return [Case(*key, why) for key, why in t.items()]


CASES = _table()
BY_ID = {case_id(c): c for c in CASES}
GEOMS = {c[:6] for c in CASES}
SHIFTED = [c for c in CASES if c.shift]
RAGGED = {"fwd-mfma": "b1-67x67-h1-ws1-s0", "bwd-mfma": "b1-66x66-h1-ws2-s1", "bwd-valu": "b1-17x19-h16-ws1-s0"}
# the geometries whose buffers the canary test guards: NT 1 .. 4, a single window, the nine regions, odd heads
CANARY = ["b1-2x2-h2-ws1-s0", "b1-7x7-h2-ws7-s3", "b1-10x10-h2-ws5-s2", "b1-12x12-h2-ws6-s5", "b1-14x14-h3-ws7-s3", "b5-5x5-h2-ws5-s0"]
# numeric regime only: an all-zero q row and an all-zero k row (the max(|x|, 1e-12) clamp)
ZERO_ROW_GEOM = Case(1, 10, 10, 2, 5, 2, "an all-zero q row and an all-zero k row: the max(|x|, 1e-12) clamp")
ZERO_Q_PIXEL, ZERO_K_PIXEL = 13, 58


# ---------------------------------------------------------------------------------------------------------------- permutations
def affine_perms(n):
    """every i -> (a i + c) mod n with gcd(a, n) = 1 except the identity, as rows of an int64 tensor (n = 1: the identity alone)"""
    if n == 1:
        return torch.zeros((1, 1), dtype=torch.int64)
    i = torch.arange(n)
    rows = [(a * i + c) % n for a in range(1, n) if math.gcd(a, n) == 1 for c in range(n) if (a, c) != (1, 0)]
    return torch.stack(rows)


def _seed(c, salt):
    return zlib.crc32(("%s/%s" % (case_id(c), salt)).encode())


@functools.lru_cache(maxsize=None)
def index_maps(cid):
    c = BY_ID.get(cid, ZERO_ROW_GEOM)
    return window_index(c.b, c.H, c.W, c.ws, c.shift, device="cpu")


@functools.lru_cache(maxsize=None)
def permutations(cid):
    """-> (pi [heads, n], rho [heads, n]) of a case: pi different per head while the family lasts; rho(i) != pi(i) everywhere, chosen
    per head so that (shifted cases) the mask decides some queries and leaves others.  rho is None when n = 1."""
    c = BY_ID[cid]
    n = n_of(c)
    cand = affine_perms(n)
    region = torch.unique(index_maps(cid)[1], dim=0)                         # distinct region patterns of the windows [u, n]
    used, pi, rho = set(), [], []
    for h in range(c.heads):
        k = (37 * h + 5) % len(cand)
        while k in used and len(used) < len(cand):
            k = (k + 1) % len(cand)
        used.add(k)
        pi.append(cand[k])
        if n == 1:
            continue
        other = region[:, pi[h]] != region                                   # pi(i) in another region than i
        best, best_score = None, -1
        for step in range(len(cand)):
            r = cand[(53 * h + 11 + step) % len(cand)]
            if bool((r == pi[h]).any()):
                continue
            by_mask = int((other & (region[:, r] == region)).sum())
            score = min(by_mask, region.numel() - by_mask)
            if score > best_score:
                best, best_score = r, score
            if score > 0 or not c.shift:
                break
        rho.append(best)
    return torch.stack(pi), (torch.stack(rho) if n > 1 else None)


# ---------------------------------------------------------------------------------------------------------------- operands
def _ints(gen, shape, hi):
    """non-zero integers of magnitude 1 .. hi"""
    mag = torch.randint(1, hi + 1, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).float()


def regimes_of(c):
    """A everywhere; B and R where the mask exists; S where there are two heads to tell apart and two keys to choose from"""
    return ("A",) + (("B", "R") if c.shift else ()) + (("S",) if c.heads >= 2 and n_of(c) > 1 else ())


@functools.lru_cache(maxsize=None)
def operands(cid, regime):
    """CPU operands and closed-form expectations of one regime of a case (fp32 tensors whose every element bf16 holds):
    qkv [pixels, 3C], dout [pixels, C], bias [heads, n, n], scale [heads], pix / region [nwin, n], sel [nwin, heads, n] (the key every
    query selects), out [pixels, C], dv [pixels, C] (exact sums), dv_stored (as bf16 stores them), dv_colsum [C] (of dv_stored)"""
    c = BY_ID[cid]
    n, heads, C = n_of(c), c.heads, 32 * c.heads
    npix = c.b * c.H * c.W
    gen = torch.Generator().manual_seed(_seed(c, regime))
    pix, region = index_maps(cid)
    nw = pix.shape[0]
    flat = pix.reshape(-1)
    pi, rho = permutations(cid)
    rows = torch.arange(n)
    bias = torch.full((heads, n, n), BIAS_OFF)
    if regime == "S":
        pow2 = lambda: 2.0 ** torch.randint(-1, 3, (nw, n, heads, 1), generator=gen).float()
        K = torch.nn.functional.one_hot(rows % 32, 32).float()[None, :, None, :] * pow2()
        Q = torch.stack([torch.nn.functional.one_hot(rho[h] % 32, 32).float() for h in range(heads)], 1)[None] * pow2()
        qk = torch.empty((npix, 2 * C))
        qk[flat] = torch.cat([Q.reshape(nw * n, C), K.reshape(nw * n, C)], 1)
        scale = torch.tensor([SCALES_S[h % 2] for h in range(heads)])
    else:
        qk = torch.randn((npix, 2 * C), generator=gen).bfloat16().float()
        scale = torch.tensor([SCALES[h % len(SCALES)] for h in range(heads)])
    assert float(qk.view(npix, 2 * heads, 32).norm(dim=-1).min()) >= 0.5     # no zero (or nearly zero) q / k row
    v = _ints(gen, (npix, C), V_MAX)
    dout = _ints(gen, (npix, C), DO_MAX)
    if regime == "R":
        dout = torch.where(torch.rand((npix, C), generator=gen) < 0.5, dout.sign() * DO_BIG, dout.sign())
    sel = pi[None].expand(nw, heads, n).clone()
    for h in range(heads):
        if regime != "A":
            bias[h, rows, rho[h]] = BIAS_S if regime == "S" else BIAS_RHO
        bias[h, rows, pi[h]] = 0.0
        if regime in ("B", "R"):
            by_mask = (region[:, pi[h]] != region) & (region[:, rho[h]] == region)
            sel[:, h] = torch.where(by_mask, rho[h][None], pi[h][None])
        if regime == "S":                                                    # integer logits: the arg-max is the closed form
            cos = ((rho[h] % 32)[:, None] == (rows % 32)[None, :]).double()
            masked = (region[:, :, None] != region[:, None, :]).double()
            sel[:, h] = (float(scale[h]) * cos[None] + bias[h].double()[None] - 100.0 * masked).argmax(-1)
    idx = sel.permute(0, 2, 1)[..., None].expand(-1, -1, -1, 32)            # [nwin, i, heads, 32] -> key of query i
    V = v[flat].view(-1, n, heads, 32)
    G = dout[flat].view(-1, n, heads, 32)
    out = torch.empty((npix, C))
    out[flat] = torch.gather(V, 1, idx).reshape(-1, C)
    dv = torch.empty((npix, C))
    dv[flat] = torch.zeros_like(G).scatter_add_(1, idx, G).reshape(-1, C)
    stored = dv.bfloat16().float()
    return dict(qkv=torch.cat([qk, v], 1), dout=dout, bias=bias, scale=scale, pix=pix, region=region, sel=sel, pi=pi, rho=rho, out=out, dv=dv,
                dv_stored=stored, dv_colsum=stored.sum(0))


def numeric_operands(c, seed=91, zero_rows=False):
    """random operands as tests/test_bench_launches_gpu._attn_inputs makes them (bf16-held q, k, v and dO of unit variance, bias
    16 sigmoid(.), scale in [5, 20]), on the CPU"""
    n, C, npix = n_of(c), 32 * c.heads, c.b * c.H * c.W
    gen = torch.Generator().manual_seed(seed + _seed(c, "numeric") % 100000)
    qkv = torch.randn((npix, 3 * C), generator=gen).bfloat16().float()
    bias = 16 * torch.sigmoid(torch.randn((c.heads, n, n), generator=gen))
    scale = 5 + 15 * torch.rand(c.heads, generator=gen)
    dout = torch.randn((npix, C), generator=gen).bfloat16().float()
    if zero_rows:
        qkv[ZERO_Q_PIXEL, :32] = 0
        qkv[ZERO_K_PIXEL, C + 32:C + 64] = 0
    return qkv, bias, scale, dout


# ---------------------------------------------------------------------------------------------------------------- float64 attention
def attention64(qkv, bias, scale, pix, region, heads):
    """the cosine window attention in float64, no operand rounding, differentiable: out [pixels, C] and the probabilities [nwin, heads,
    n, n].  softmax(normalize(q) normalize(k)^T scale_h + bias_h - 100 [region_i != region_j]) v, x / max(|x|, 1e-12)."""
    nw, n = pix.shape
    C = 32 * heads
    X = qkv.double()[pix.reshape(-1)].view(nw, n, 3, heads, 32).permute(2, 0, 3, 1, 4)
    q, k, v = X[0], X[1], X[2]
    qh = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    kh = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    masked = (region[:, None, :, None] != region[:, None, None, :]).double()
    logit = qh @ kh.transpose(-1, -2) * scale.double().view(1, heads, 1, 1) + bias.double().view(1, heads, n, n) - 100.0 * masked
    P = torch.softmax(logit, -1)
    O = (P @ v).permute(0, 2, 1, 3).reshape(nw * n, C)
    out = torch.zeros((qkv.shape[0], C), dtype=torch.float64).index_put((pix.reshape(-1),), O)
    return out, P, logit


def attention64_grads(qkv, dout, bias, scale, pix, region, heads):
    """-> out, dqkv, dbias, dscale (float64, detached) and the probabilities / logits"""
    q = qkv.double().clone().requires_grad_(True)
    b = bias.double().clone().requires_grad_(True)
    s = scale.double().clone().requires_grad_(True)
    out, P, logit = attention64(q, b, s, pix, region, heads)
    out.backward(dout.double())
    return out.detach(), q.grad, b.grad, s.grad, P.detach(), logit.detach()
