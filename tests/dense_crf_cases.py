"""Named frames for the permutohedral dense CRF's edge tests (tests/test_gpu_dense_crf_permutohedral_edges.py): each case is an image
builder, a size and the three standard deviations, chosen for one path of csrc/dense_crf_permutohedral.hip -- a second round of the
scans over sort tiles, an odd or even number of radix passes, long or short contributor lists in the chunked splat, frames below one
chunk or one tile.  tests/test_dense_crf_cases_host.py asserts on the CPU that every case still has the property it was chosen for, so
that a later edit of a builder cannot quietly empty a GPU test.  The references stay in tests/test_dense_crf_permutohedral.py."""
import math
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from tests.test_dense_crf import blocky_image, g

F32 = np.float32
TILE = 2048   # elements per sort tile (ST * SI of the kernel file)
CH = 64       # contributors per splat chunk


class Case(NamedTuple):
    H: int
    W: int
    image: Callable[[int], torch.Tensor]   # frame number -> u8 [H, W, 3]
    pos_xy: float = 1.0
    bi_xy: float = 67.0
    bi_rgb: float = 3.0

    @property
    def stds(self):
        return dict(pos_xy_std=self.pos_xy, bi_xy_std=self.bi_xy, bi_rgb_std=self.bi_rgb)

    def E(self, d):
        return self.H * self.W * (d + 1)

    def NT(self, d):
        return (self.E(d) + TILE - 1) // TILE


def _blocky(H, W, seed, noise=4):
    return lambda b=0: blocky_image(H, W, seed + b, noise=noise)


def _constant(H, W):
    return lambda b=0: torch.tensor([90 + b, 140, 200], dtype=torch.uint8).expand(H, W, 3).contiguous()


def _random(H, W, seed):
    return lambda b=0: torch.randint(0, 256, (H, W, 3), generator=g(seed + b), dtype=torch.uint8)


def _checker(H, W):
    """0 / 255 per pixel, the corners pure red, green, blue (and white): every colour coordinate at both ends of its range."""
    def build(b=0):
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        img = (((ys + xs + b) % 2) * 255).to(torch.uint8)[..., None].expand(H, W, 3).contiguous()
        img[0, 0] = torch.tensor([255, 0, 0], dtype=torch.uint8)
        img[0, W - 1] = torch.tensor([0, 255, 0], dtype=torch.uint8)
        img[H - 1, 0] = torch.tensor([0, 0, 255], dtype=torch.uint8)
        img[H - 1, W - 1] = torch.tensor([255, 255, 255], dtype=torch.uint8)
        return img
    return build


CASES = {
    # A: the smallest frames whose lattices have more than 256 sort tiles (a second round of the digit and tile scans)
    "tiles_bilateral": Case(283, 309, _blocky(283, 309, 283)),
    "tiles_gaussian": Case(419, 421, _blocky(419, 421, 419)),
    # B: radix pass counts of the bilateral lattice: 5 (pydensecrf's own defaults), 7 and 4.  A one-pass sort is not reachable: the
    # slack of the host's range bound keeps every coordinate at 5 bits or more, so the Gaussian lattice alone has >= 10 bits.
    "passes_5": Case(40, 56, _blocky(40, 56, 5), 3.0, 80.0, 13.0),
    "passes_7": Case(40, 56, _blocky(40, 56, 7), 0.5, 20.0, 1.0),
    "passes_4": Case(40, 56, _blocky(40, 56, 4), 40.0, 200.0, 60.0),
    # C: contributor lists per lattice point, from one frame-wide list to none longer than 2
    "constant": Case(64, 64, _constant(64, 64)),
    "flat_blocks": Case(64, 64, _blocky(64, 64, 64, noise=0)),
    "random": Case(64, 64, _random(64, 64, 64)),
    "wide_gaussian": Case(64, 64, _blocky(64, 64, 40), pos_xy=40.0),
    "checker": Case(33, 47, _checker(33, 47)),
    "checker_narrow": Case(33, 47, _checker(33, 47), 1.0, 20.0, 1.0),
    # D: below one tile; 3 x 5 is below one chunk for the Gaussian lattice, 2 x 11 has one chunk position and 2 contributors past it
    "tiny_1x1": Case(1, 1, _blocky(1, 1, 1)),
    "tiny_1x70": Case(1, 70, _blocky(1, 70, 2)),
    "tiny_70x1": Case(70, 1, _blocky(70, 1, 3)),
    "tiny_3x5": Case(3, 5, _blocky(3, 5, 4)),
    "tiny_2x11": Case(2, 11, _blocky(2, 11, 5)),
    # E: the shared pass (frames b = 0..2)
    "shared": Case(37, 45, _blocky(37, 45, 30)),
    # F: the frame of the 32-column debug-row test, for the 64-column layout
    "blocky64": Case(64, 64, _blocky(64, 64, 128)),
}
TINY = ("tiny_1x1", "tiny_1x70", "tiny_70x1", "tiny_3x5", "tiny_2x11")


def chunk_stats(lat):
    """Per lattice point of ``lat`` (lattice32's dict; only ``vert`` is read): the number of contributors, and the number of aligned
    blocks of 64 sorted positions that lie inside the point's range [s, e) of the sorted order -- splat_sum's c1 - c0 with
    c0 = ceil(s / 64), c1 = floor(e / 64) (0 where c0 >= c1).  The sort orders the vertices by point, so s is the count before."""
    vert = np.asarray(lat["vert"]).reshape(-1)
    count = np.bincount(vert, minlength=int(lat["M"]) + 1)[1:]
    e = np.cumsum(count)
    s = e - count
    chunks = np.maximum(e // CH - (s + CH - 1) // CH, 0)
    return count, chunks


def key_bits(d, H, W, xy_std, rgb_std=None) -> Optional[int]:
    """The packed key width lattice_setup derives for a d-dimensional lattice (its radix sort runs ceil(bits / 8) passes), or None
    where it refuses the range.  A plain transcription of the host code, used only to assert that a case has the pass count it was
    chosen for: a coverage condition, not a correctness check (the sort is checked through the lattice it produces)."""
    sxy = F32(xy_std)
    inv_std_dev = F32(math.sqrt(2.0 / 3.0) * (d + 1))
    fmax = [float(F32(W - 1) / sxy), float(F32(H - 1) / sxy)] + [float(F32(255.0) / F32(rgb_std))] * (d - 2) if d > 2 else \
        [float(F32(W - 1) / sxy), float(F32(H - 1) / sxy)]
    C = [0.0] * (d + 1)
    for i in range(d):
        scale = F32(1.0 / math.sqrt(float((i + 2) * (i + 1))) * float(inv_std_dev))
        C[i + 1] = fmax[i] * float(scale) * (1 + 1e-6)
    slack = 3.0 * (d + 1) + 2
    total = 0
    for j in range(d):
        hi = sum(C[j + 1:])
        lo = 0.0 if j == 0 else -float(j) * C[j]
        clo, chi = math.floor(lo - slack), math.ceil(hi + slack)
        if clo < -32768 or chi > 32767:
            return None
        span = int(chi - clo) + 1
        bits = 1
        while (1 << bits) < span:
            bits += 1
        total += bits
    return None if total > 64 else total


def passes(bits):
    return (bits + 7) // 8
