"""Inputs shared by tests/test_rectify_host.py and tests/test_gpu_rectify.py: the test cameras, the maps with the tap classes each one
is used to cover, seeded source frames of every kind, and the C-ABI calls that must be refused.  The host file checks the coverage
claims on the CPU, so the GPU file can rely on them."""
import ctypes as C

import numpy as np

import rectify_ref as R

SRC = (33, 47)                      # (H, W): "the Hoengg camera at 47 x 33"
SIZES = ((3, 3), (4, 6), (7, 5), (33, 47))
PLUMB_BOB_D = (-0.28, 0.07, 0.001, -0.0005, 0.0)
MIN_CLASS = 20                      # a map covers a tap class only with at least this many pixels of it


def halved(K):
    Kh = K.copy()
    Kh[0, 0] *= 0.5
    Kh[1, 1] *= 0.5
    return Kh


def plumb_bob_K(H, W):
    return np.array([[0.6 * W, 0, W / 2 - 0.5 + 1.3], [0, 0.6 * W, H / 2 - 0.5 - 0.7], [0, 0, 1]], dtype=np.float64)


def camera_maps(H=SRC[0], W=SRC[1]):
    """{name: (rectify_map arguments as a dict, classes the map is claimed to cover)} for the H x W Hoengg camera."""
    K = R.hoengg(W, H)

    def eq(out, Kn):
        return dict(K=K, D=R.HOENGG_D, model="equidistant", src_size=(H, W), out_size=out,
                    new_K=np.diag([out[1] / W, out[0] / H, 1.0]) @ Kn)

    maps = {
        "K": (eq((H, W), K), ("full", "partial")),
        "half": (eq((H, W), halved(K)), ("full", "partial", "none")),
        "K_28x20": (eq((20, 28), K), ("full", "partial")),
        "half_28x20": (eq((20, 28), halved(K)), ("full", "none")),
        "plumb_bob": (dict(K=plumb_bob_K(H, W), D=PLUMB_BOB_D, model="plumb_bob", src_size=(H, W), out_size=None, new_K=None), ("full",)),
    }
    for w in (1, 3, 5):   # the vector-store tail, and rows shorter than one thread's span
        maps[f"K_w{w}"] = (eq((20, w), K), ())
        maps[f"half_w{w}"] = (eq((20, w), halved(K)), ())
    return maps


def crop_448(K):
    """K_new of the centre crop of the 1440 x 1080 frame to 1080 x 1080, scaled to 448 x 448."""
    s = 448 / 1080
    return np.array([[K[0, 0] * s, 0, (K[0, 2] - (1440 - 1080) / 2) * s], [0, K[1, 1] * s, K[1, 2] * s], [0, 0, 1]], dtype=np.float64)


def source_frames(encoding, B, H, W, pad=0, seed=0):
    """(uint8 [B, rows * step] bytes with random padding, step): B different frames of `encoding`."""
    rng = np.random.default_rng([seed, B, H, W, pad, R.ENCODINGS.index(encoding)])
    step = W * R.bytes_per_pixel(encoding) + pad
    rows = 3 * H if encoding == "planar" else H
    return rng.integers(0, 256, (B, rows * step), dtype=np.uint8), step


def mosaic_of(rgb, pattern):
    """uint8 [3,H,W] -> the uint8 [H,W] mosaic a `pattern` sensor sees of it."""
    ry, rx = R.BAYER[pattern]
    _, H, W = rgb.shape
    yy, xx = np.mgrid[0:H, 0:W]
    red_row = (yy & 1) == ry
    own = ((xx & 1) == rx) == red_row
    return np.where(own, np.where(red_row, rgb[0], rgb[2]), rgb[1]).astype(np.uint8)


def abi_refusals(h):
    """[(what, return code)] of calls wvn_unpack_frames / wvn_rectify_frames must refuse before any launch.  The pointers are host
    words that a refused call never dereferences."""
    words = (C.c_longlong * 8)()
    p = C.addressof(words)

    def unpack(src=p, kind=0, B=1, H=8, W=8, step=8, stride=64, out=p, order=0):
        return h.wvn_unpack_frames(src, kind, B, H, W, step, stride, out, order, None)

    def rect(src=p, kind=0, B=1, H=8, W=8, step=8, stride=64, qx=p, qy=p, hh=4, ww=4, out=p, order=0):
        return h.wvn_rectify_frames(src, kind, B, H, W, step, stride, qx, qy, hh, ww, out, order, None)

    calls = []
    for name, f in (("unpack", unpack), ("rectify", rect)):
        calls += [(f"{name}: null source", f(src=None)), (f"{name}: null output", f(out=None)),
                  (f"{name}: B = 0", f(B=0)), (f"{name}: H = 0", f(H=0, stride=8)), (f"{name}: W = 0", f(W=0)),
                  (f"{name}: a 2-row mosaic", f(kind=4, H=2, stride=16)), (f"{name}: a 2-column mosaic", f(kind=7, W=2)),
                  (f"{name}: step below a row", f(step=7)), (f"{name}: step below a packed row", f(kind=1, step=23, stride=23 * 8)),
                  (f"{name}: frame stride below a frame", f(stride=63)),
                  (f"{name}: planar frame stride of one plane", f(kind=3, stride=64)),
                  (f"{name}: kind -1", f(kind=-1)), (f"{name}: kind 8", f(kind=8)), (f"{name}: order 3", f(order=3)),
                  (f"{name}: gray order on a colour source", f(kind=1, step=24, stride=192, order=2)),
                  (f"{name}: source bytes past 31 bits", f(B=3, H=1024, W=1024, step=1 << 20, stride=1 << 30)),
                  (f"{name}: a side above the limit", f(H=1, W=65536, step=65536, stride=65536))]
    calls += [("unpack: output bytes past 31 bits", unpack(B=50, H=4096, W=4096, step=4096, stride=1 << 24, order=1)),
              ("rectify: null map", rect(qx=None)), ("rectify: null map y", rect(qy=None)), ("rectify: h = 0", rect(hh=0)),
              ("rectify: w = 0", rect(ww=0)), ("rectify: map bytes past 31 bits", rect(hh=32768, ww=32768)),
              ("rectify: output bytes past 31 bits", rect(B=50, hh=4096, ww=4096, order=1))]
    assert all(v == 0 for v in words)
    return calls
