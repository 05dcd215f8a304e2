"""Plain statement of the random-pixel sampler of csrc/random_pixels.hip (ops.random_pixels) in numpy integer arithmetic:
the keyed bijection pi of [0, H*W), its inverse, and the two outputs ``idx`` and ``seg``.  A helper, not collected as tests.

    key        (seed, frame), both unsigned 32-bit; frame = (frame0 + b) mod 2^32 for image b of a batch
    round keys the high 32 bits of four successive splitmix64 outputs from the state seed << 32 ^ frame
    network    balanced Feistel on 2n bits, 4^n the smallest such power >= H*W, four rounds:
               (L, R) -> (R, L ^ (fmix32(R ^ k_i) & (2^n - 1))),  fmix32 = murmur3's 32-bit finaliser
    pi         cycle walking: apply the network until the value is < H*W (a bijection of [0, 4^n) restricted this way is a
               bijection of [0, H*W); its inverse walks the inverse network)
    idx[j]     = pi(j)             for j < nr
    seg[p]     = pi^-1(p) if that is < nr, else -1

No torch generator is involved: the samples are a function of (seed, frame, H*W) alone."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
ROUNDS = 4


def splitmix64(state: int):
    """One step: (new state, output), Python integers modulo 2^64."""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def round_keys(seed: int, frame: int):
    state = ((seed & M32) << 32) ^ (frame & M32)
    keys = []
    for _ in range(ROUNDS):
        state, z = splitmix64(state)
        keys.append(z >> 32)
    return keys


def half_bits(n_pix: int) -> int:
    n = 0
    while (1 << (2 * n)) < n_pix:
        n += 1
    return n


def fmix32(h: np.ndarray) -> np.ndarray:
    """murmur3's finaliser on uint64 arrays holding 32-bit values."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def _network(x: np.ndarray, keys, n: int, inverse: bool) -> np.ndarray:
    mask = np.uint64((1 << n) - 1)
    L, R = x >> np.uint64(n), x & mask
    if not inverse:
        for k in keys:
            L, R = R, L ^ (fmix32(R ^ np.uint64(k)) & mask)
    else:
        for k in reversed(keys):
            L, R = R ^ (fmix32(L ^ np.uint64(k)) & mask), L
    return (L << np.uint64(n)) | R


def _walk(x, n_pix: int, seed: int, frame: int, inverse: bool) -> np.ndarray:
    keys, n = round_keys(seed, frame), half_bits(n_pix)
    x = np.atleast_1d(np.asarray(x)).astype(np.uint64)
    assert (x < np.uint64(n_pix)).all()
    out = _network(x, keys, n, inverse)
    while True:
        todo = out >= np.uint64(n_pix)
        if not todo.any():
            return out.astype(np.int64)
        out[todo] = _network(out[todo], keys, n, inverse)


def pi(j, n_pix: int, seed: int, frame: int) -> np.ndarray:
    return _walk(j, n_pix, seed, frame, False)


def pi_inv(p, n_pix: int, seed: int, frame: int) -> np.ndarray:
    return _walk(p, n_pix, seed, frame, True)


def random_pixels(batch: int, H: int, W: int, nr: int, seed: int = 0, frame0: int = 0):
    """-> (idx [B, nr] int32, seg [B, H, W] int32): what ops.random_pixels returns."""
    assert 1 <= nr <= H * W <= (1 << 30)
    idx = np.empty((batch, nr), dtype=np.int32)
    seg = np.empty((batch, H, W), dtype=np.int32)
    for b in range(batch):
        frame = (frame0 + b) & M32
        idx[b] = pi(np.arange(nr), H * W, seed, frame)
        q = pi_inv(np.arange(H * W), H * W, seed, frame)
        seg[b] = np.where(q < nr, q, -1).reshape(H, W)
    return idx, seg
