"""float64 references of the implicit-GEMM convolutions (GPU, chunked over images; no library convolution involved) and the window
partition of SwinV2's shifted-window attention.  Shared by tests/test_poisoned_kernels_gpu.py and tests/test_bench_launches_gpu.py."""
import torch
import torch.nn.functional as F


def ref_conv(x, w, stride, pad, chunk=16):
    """x [N,H,W,C], w [K,R,S,C] -> float64 y [N,Ho,Wo,K] (unfold + GEMM over image chunks: no library convolution involved)"""
    n, h, wd, c = x.shape
    k, r, s, _ = w.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - s) // stride + 1
    wm = w.double().permute(0, 3, 1, 2).reshape(k, c * r * s)
    out = torch.empty((n, ho, wo, k), dtype=torch.float64, device=x.device)
    for i in range(0, n, chunk):
        xc = x[i:i + chunk].double().permute(0, 3, 1, 2)
        cols = F.unfold(xc, (r, s), padding=pad, stride=stride)                   # [b, C*R*S, L]
        out[i:i + chunk] = (wm @ cols).view(xc.shape[0], k, ho, wo).permute(0, 2, 3, 1)
    return out


def ref_dgrad(dy, w, x_shape, stride, pad, chunk=16):
    n, h, wd, c = x_shape
    k, r, s, _ = w.shape
    wm = w.double().permute(0, 3, 1, 2).reshape(k, c * r * s)
    out = torch.empty((n, h, wd, c), dtype=torch.float64, device=dy.device)
    for i in range(0, n, chunk):
        d = dy[i:i + chunk].double()
        b, ho, wo, _ = d.shape
        cols = wm.t() @ d.reshape(b, ho * wo, k).transpose(1, 2)                  # [b, C*R*S, L]
        out[i:i + chunk] = F.fold(cols, (h, wd), (r, s), padding=pad, stride=stride).permute(0, 2, 3, 1)
    return out


def ref_wgrad(dy, x, r, s, stride, pad, chunk=16):
    n, h, wd, c = x.shape
    k = dy.shape[3]
    acc = torch.zeros((k, c * r * s), dtype=torch.float64, device=x.device)
    for i in range(0, n, chunk):
        xc = x[i:i + chunk].double().permute(0, 3, 1, 2)
        cols = F.unfold(xc, (r, s), padding=pad, stride=stride)
        d = dy[i:i + chunk].double()
        acc += torch.einsum("blk,bcl->kc", d.reshape(d.shape[0], -1, k), cols)
    return acc.view(k, c, r, s).permute(0, 2, 3, 1)                                # [K,R,S,C]


def window_index(b, H, W, ws, shift, device="cuda"):
    """pixel [nwin, ws*ws] (row of an [b*H*W, C] tensor) and shift-mask region [nwin, ws*ws] of every token of every window: window
    (wy, wx) of image i of the image rolled by -shift in both directions, tokens row-major, regions 3 x 3 by the slices [0, H-ws),
    [H-ws, H-shift), [H-shift, H) of the rolled image (all 0 without a shift).  Formed arithmetically; tests/test_ref64_cpu.py holds it to
    the torch.roll + window-partition construction."""
    wpr, wpc = W // ws, H // ws
    win = torch.arange(b * wpc * wpr, device=device)
    bi, r = win // (wpc * wpr), win % (wpc * wpr)
    wy, wx = r // wpr, r % wpr
    tok = torch.arange(ws * ws, device=device)
    ty, tx = tok // ws, tok % ws
    hs, wsx = wy[:, None] * ws + ty[None], wx[:, None] * ws + tx[None]
    pix = (bi[:, None] * H + (hs + shift) % H) * W + (wsx + shift) % W
    if shift:
        rh = torch.where(hs < H - ws, 0, torch.where(hs < H - shift, 1, 2))
        rw = torch.where(wsx < W - ws, 0, torch.where(wsx < W - shift, 1, 2))
        region = rh * 3 + rw
    else:
        region = torch.zeros_like(pix)
    return pix, region
