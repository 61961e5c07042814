"""The window partition the float64 attention reference uses (tests/ref64.window_index) against the standard shifted-window construction:
torch.roll by -shift, window partition, and the attention mask built from the three slices per axis of the rolled image."""
import pytest
import torch

from ref64 import window_index


def partition(x, ws):
    """[b, H, W] -> [b * (H / ws) * (W / ws), ws * ws], windows row-major per image, tokens row-major per window"""
    b, H, W = x.shape
    return x.view(b, H // ws, ws, W // ws, ws).permute(0, 1, 3, 2, 4).reshape(-1, ws * ws)


@pytest.mark.parametrize("geom", [(2, 12, 12, 6, 3), (3, 6, 6, 3, 1), (2, 14, 21, 7, 3), (2, 12, 12, 6, 0),
                                  # one-token, 2 x 2, full-tile and two-tile windows; H != W both ways; H == ws (no slice 0 on that
                                  # axis); the smallest and the largest shift
                                  (2, 2, 3, 1, 0), (1, 4, 6, 2, 1), (2, 8, 8, 4, 3), (1, 4, 4, 4, 1), (1, 10, 15, 5, 4), (1, 15, 5, 5, 1),
                                  (2, 5, 5, 5, 2), (1, 7, 7, 7, 3), (1, 7, 14, 7, 6), (1, 21, 7, 7, 1), (1, 12, 12, 6, 5), (1, 2, 2, 2, 1)])
def test_window_index_is_the_rolled_partition_with_the_slice_mask(geom):
    b, H, W, ws, shift = geom
    pix, region = window_index(b, H, W, ws, shift, device="cpu")
    ids = torch.arange(b * H * W).view(b, H, W)
    rolled = torch.roll(ids, shifts=(-shift, -shift), dims=(1, 2)) if shift else ids
    assert torch.equal(pix, partition(rolled, ws))
    img = torch.zeros((1, H, W), dtype=torch.long)
    if shift:
        cnt = 0
        for hsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hsl, wsl] = cnt
                cnt += 1
    want = partition(img.expand(b, H, W).contiguous(), ws)
    assert torch.equal(region, want)
    # the mask the attention applies (-100 between tokens of different regions) is the same either way
    assert torch.equal(region[:, :, None] != region[:, None, :], want[:, :, None] != want[:, None, :])
