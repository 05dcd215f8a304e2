"""The plain statement of connectivity enforcement (include/wvn_hip.h: wvn_slic_connectivity), written to be obviously right and not
fast.  It is the oracle of tests/test_slic_connectivity_host.py and tests/test_gpu_slic_connectivity.py; the kernels never serve as
their own reference.

    1. A component is a maximal 4-connected set of pixels with equal label; its size is its pixel count.
    2. A component is anchored if its size is >= min_size.  If no component is anchored, the output is the input.
    3. Round: every decision reads the state at the start of the round.  For every component C that is not yet anchored, take all pairs
       (p, q) with p in C, q a 4-neighbour of p inside the frame, q anchored.  No such pair: C waits.  Otherwise count the pairs per
       current label of q; C takes the label with the highest count, the lowest id on a tie, and is anchored from the next round on.
    4. Rounds repeat until every pixel is anchored.
"""
import numpy as np
from scipy import ndimage


def components(labels: np.ndarray):
    """-> (comp [H,W] int64 ids 0..n-1, sizes [n]); scipy's default structuring element is the cross: 4-connectivity."""
    comp = np.zeros(labels.shape, dtype=np.int64)
    n = 0
    for k in np.unique(labels):
        c, m = ndimage.label(labels == k)
        comp[c > 0] = c[c > 0] + n - 1
        n += m
    return comp, np.bincount(comp.ravel(), minlength=n)


def small_components(labels: np.ndarray, min_size: int) -> int:
    """Number of 4-connected components below min_size."""
    return int((components(labels)[1] < min_size).sum())


def min_size_for(H: int, W: int, n_clusters: int, factor: float = 0.25) -> int:
    return max(1, int(factor * H * W / n_clusters))


def enforce_connectivity(labels: np.ndarray, min_size: int, return_rounds: bool = False):
    """labels [H,W] integer -> int32 [H,W] (and the number of rounds that changed something)."""
    L = np.asarray(labels).astype(np.int64)
    H, W = L.shape
    comp, sizes = components(L)                      # two waiting components of one label never touch: this labelling serves all rounds
    anchored = sizes[comp] >= min_size               # per pixel
    rounds = 0
    if not anchored.any():
        out = L.astype(np.int32)
        return (out, 0) if return_rounds else out
    cur = L.copy()
    waiting = [c for c in range(len(sizes)) if sizes[c] < min_size]
    pix = {c: np.argwhere(comp == c) for c in waiting}
    while waiting:
        decided = {}
        for c in waiting:
            votes = {}
            for y, x in pix[c]:
                for qy, qx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= qy < H and 0 <= qx < W and anchored[qy, qx]:
                        votes[cur[qy, qx]] = votes.get(cur[qy, qx], 0) + 1
            if votes:
                top = max(votes.values())
                decided[c] = min(k for k, v in votes.items() if v == top)
        assert decided, "the pixel grid is connected: some waiting component touches an anchored one"
        for c, k in decided.items():                 # applied after every decision of the round has been made
            ys, xs = pix[c][:, 0], pix[c][:, 1]
            cur[ys, xs] = k
            anchored[ys, xs] = True
        waiting = [c for c in waiting if c not in decided]
        rounds += 1
    out = cur.astype(np.int32)
    return (out, rounds) if return_rounds else out


# ---- hand-written maps: (name, map, min_size, expected), every answer worked out by hand ---------------------------------------------
def hand_cases():
    cases = []
    # a one-pixel island of 1 inside 0 -> 0
    a = np.zeros((5, 5), dtype=np.int32); a[2, 2] = 1
    cases.append(("island", a, 4, np.zeros((5, 5), dtype=np.int32)))
    # an island (2, one pixel) inside an island (1, a ring of 8) inside a superpixel (0, 40 pixels): round 1: the ring (size 8 < 9)
    # takes 0, the inner pixel touches only the ring, which is not anchored yet, and waits; round 2: it takes what the ring took
    b = np.zeros((7, 7), dtype=np.int32); b[2:5, 2:5] = 1; b[3, 3] = 2
    cases.append(("nested", b, 9, np.zeros((7, 7), dtype=np.int32)))
    # a fragment between two anchored superpixels with equal border length: columns 0-1 are id 3, column 2 is a fragment (id 7, 4
    # pixels), columns 3-4 are id 1; 4 pairs each way -> the lowest id, 1
    c = np.empty((4, 5), dtype=np.int32); c[:, :2] = 3; c[:, 2] = 7; c[:, 3:] = 1
    e = c.copy(); e[:, 2] = 1
    cases.append(("tie", c, 5, e))
    # a fragment in the frame's corner: pixel (0,0) = 2 with 1 to its right, 0 below; out-of-frame neighbours do not vote, so it is a
    # 1 : 1 tie -> 0; (with votes from outside the frame anything else could win)
    d = np.zeros((4, 4), dtype=np.int32); d[0, 1:] = 1; d[1, 1:] = 1; d[0, 0] = 2
    e = d.copy(); e[0, 0] = 0
    cases.append(("corner", d, 3, e))
    # a fragment that touches two anchored components of the SAME label: rows 0-1 are one component of id 6, rows 3-4 another (row 2 holds
    # no 6, so they are separate); row 2 is [5 5 9 7 7].  The fragment (2,2) has one pair with each: label 6 gets 1 + 1 = 2 pairs, 5 and
    # 7 one each -> 6.  (Counted per component instead of per label, all four would tie at 1 and the lowest id, 5, would win.)
    f = np.full((5, 5), 6, dtype=np.int32); f[2] = [5, 5, 9, 7, 7]
    e = f.copy(); e[2, 2] = 6
    cases.append(("same_label_twice", f, 2, e))
    # nothing below min_size: unchanged
    g = np.zeros((4, 4), dtype=np.int32); g[:, 2:] = 1
    cases.append(("all_large", g, 8, g.copy()))
    # min_size above every component: nothing is anchored, unchanged
    cases.append(("none_anchored", b, 100, b.copy()))
    return cases
