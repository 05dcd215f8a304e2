"""Degenerate inputs of the cosine k-means (oracle/interfaces.py::kmeans_cosine_labels_numpy): exact ties between similarities, clusters
that end up empty and keep their centroid, rows that are exactly zero -- what Gaussian codes never produce and what constant image
regions (sky, saturated or masked areas) do.  One input builder and one checker, plain functions without GPU or project code:

    degenerate_code   piecewise-constant integer patch codes: a 3 x 3 arrangement of constant blocks over the G x G patch grid
    describe          how degenerate such an input is, from the oracle alone

Use the builder only with (G, H) for which (G - 1) / (H - 1) is a power of two -- (9, 65), (5, 33), (17, 129): then every tap weight
of the fixed-order bilinear interpolation is dyadic, the interpolation of small integers is exact, and the pixels inside a block are
bit-identical rows (identical similarities against every centroid: exact ties wherever two centroids are equal).
"""
import numpy as np

from oracle import interfaces as OI

# (G, H, C, K, n_vectors): the fixtures tests/test_oracle_stego.py proves degenerate and tests/test_gpu_kmeans_edges.py runs
DIRECT_FIXTURES = [(9, 65, 90, 20, 5), (9, 65, 16, 6, 3), (9, 65, 90, 27, 5), (9, 65, 16, 40, 6), (17, 129, 90, 64, 6)]
LINEAR_FIXTURES = [(9, 65, 90, 20, 5), (9, 65, 90, 27, 5), (5, 33, 16, 6, 3)]
# the blocks in the order they are given their vector: (0, 0) and (1, 1) are zero, the others cycle through the non-zero vectors
_BLOCK_ORDER = [(0, 0), (1, 1), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]


def degenerate_code(G: int, C: int, n_vectors: int, seed: int) -> np.ndarray:
    """[G*G, C] fp32 patch codes: block (r, c) of the 3 x 3 arrangement (patch row i lies in block row 3 i // G) is constant; its
    vector is one of ``n_vectors`` distinct ones with integer entries in [-3, 3], the first of which is zero.  Blocks (0, 0) and (1, 1)
    are zero (constant-zero regions of more than one size), the seven others cycle through the n_vectors - 1 non-zero vectors."""
    assert 2 <= n_vectors <= 8 and G >= 3
    rng = np.random.default_rng(seed)
    while True:
        vec = rng.integers(-3, 4, size=(n_vectors, C)).astype(np.float32)
        vec[0] = 0.0
        if len(np.unique(vec, axis=0)) == n_vectors and np.abs(vec[1:]).sum(1).min() > 0:
            break
    blk = (np.arange(G) * 3) // G
    code = np.empty((G, G, C), dtype=np.float32)
    for q, (r, c) in enumerate(_BLOCK_ORDER):
        code[np.ix_(blk == r, blk == c)] = vec[0 if q < 2 else 1 + (q - 2) % (n_vectors - 1)]
    return code.reshape(G * G, C)


def describe(code: np.ndarray, G: int, H: int, K: int) -> dict:
    """{"duplicate_centroids", "zero_rows", "tie_share", "used_clusters"} of the direct statement of the pixel k-means on ``code``:
    initial centroids that repeat an earlier one bit for bit, pixel rows that are exactly zero, the share of the pixels whose two
    best first-pass similarities (the oracle's fp32 fma chains) are EQUAL, and the ids in use after the default 10 iterations."""
    dense = OI.upsample_bilinear_fixed(code.reshape(G, G, -1), H).reshape(H * H, -1)
    P = H * H
    x = OI._normalize_rows_f32(dense)
    cent = x[[((2 * k + 1) * P) // (2 * K) for k in range(K)]]
    rows, inverse = np.unique(x, axis=0, return_inverse=True)      # (the similarities of bit-identical rows are computed once)
    sim = np.sort(OI._seq_dot_f32(rows[:, None, :], cent[None, :, :]), axis=1)
    tie = (sim[:, -1] == sim[:, -2])[inverse.reshape(-1)]
    labels = OI.kmeans_cosine_labels(dense, K)
    return {"duplicate_centroids": K - len(np.unique(cent, axis=0)), "zero_rows": int((dense == 0).all(1).sum()),
            "tie_share": float(tie.mean()), "used_clusters": len(np.unique(labels))}
