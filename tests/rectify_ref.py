"""The raw camera ingest stated in numpy: the definition ops.unpack_frames / ops.rectify are held to (include/wvn_hip.h: "Raw camera
ingest").  The map is float64, everything after it is integer, so the GPU result is this one bit for bit.

    source    mono8 | rgb8 / bgr8 (packed HWC) | planar [3,H,W] | bayer_{rggb,bggr,gbrg,grbg}8, rows of `step` bytes
    demosaic  bilinear with round-half-up shifts; the one-pixel ring copies its neighbours (columns first, then rows)
    map       pinhole K_new -> R^T -> plumb_bob | equidistant -> K, clamped, quantised to Q5 (rint, ties to even)
    sampling  bilinear with 5-bit weights, taps outside the frame are 0, (sum + 512) >> 10

cv2.cvtColor(COLOR_Bayer*), cv2.initUndistortRectifyMap / cv2.fisheye and cv2.remap(INTER_LINEAR, BORDER_CONSTANT) are what these
rules aim at; that parity is NOT pinned (OpenCV is not a dependency).  Written for clarity, not speed.
"""
import math

import numpy as np

BAYER = {"bayer_rggb8": (0, 0), "bayer_bggr8": (1, 1), "bayer_gbrg8": (1, 0), "bayer_grbg8": (0, 1)}   # (row, column) of R in the 2 x 2 tile
ENCODINGS = ("mono8", "rgb8", "bgr8", "planar") + tuple(BAYER)
Q = 32          # Q5: OpenCV's INTER_BITS
SENTINEL = -2   # where a non-finite coordinate lands (in pixels): every tap is outside

# the Hoengg camera of the reference's dataset scripts (1440 x 1080, equidistant): fx, fy, cx, cy and k1..k4
HOENGG_K = (575.6050407221768, 578.564849365178, 745.7312198525915, 519.5207040671075)
HOENGG_D = (0.4316922809468283, 0.09279900476637248, -0.4010909691803734, 0.4756163338479413)
HOENGG_SIZE = (1080, 1440)


def hoengg(W: int, H: int):
    """K (3 x 3) of the Hoengg camera at W x H: fx, fy and cx scaled by W / 1440, cy by H / 1080."""
    fx, fy, cx, cy = HOENGG_K
    s = W / 1440
    return np.array([[fx * s, 0, cx * s], [0, fy * s, cy * H / 1080], [0, 0, 1]], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ sources
def bytes_per_pixel(encoding: str) -> int:
    return 3 if encoding in ("rgb8", "bgr8") else 1


def rows_of(buf, encoding: str, H: int, W: int, step=None) -> np.ndarray:
    """The bytes of one frame -> uint8 [rows, W bpp] with the padding of `step` dropped (planar: 3 H rows)."""
    bpp = bytes_per_pixel(encoding)
    step = W * bpp if step is None else step
    rows = 3 * H if encoding == "planar" else H
    a = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.reshape(-1)
    assert step >= W * bpp and a.size >= (rows - 1) * step + W * bpp
    out = np.empty((rows, W * bpp), dtype=np.uint8)
    for r in range(rows):
        out[r] = a[r * step:r * step + W * bpp]
    return out


def demosaic(raw: np.ndarray, pattern: str) -> np.ndarray:
    """uint8 [H,W] mosaic -> uint8 [3,H,W] RGB: demosaic_scalar's rules on whole arrays (a camera-sized frame in a blink)."""
    H, W = raw.shape
    assert H >= 3 and W >= 3
    ry, rx = BAYER[pattern]
    r = raw.astype(np.int32)
    c, n, s, w, e = r[1:-1, 1:-1], r[:-2, 1:-1], r[2:, 1:-1], r[1:-1, :-2], r[1:-1, 2:]
    diag = r[:-2, :-2] + r[:-2, 2:] + r[2:, :-2] + r[2:, 2:]
    yy, xx = np.mgrid[1:H - 1, 1:W - 1]
    red_row = (yy & 1) == ry
    own = ((xx & 1) == rx) == red_row                                   # an R or B site; the rest are G sites
    green = np.where(own, (n + s + e + w + 2) >> 2, c)
    mine = np.where(own, c, (w + e + 1) >> 1)                           # the colour of this row's R / B sites
    other = np.where(own, (diag + 2) >> 2, (n + s + 1) >> 1)            # the other of R and B
    out = np.zeros((3, H, W), dtype=np.int32)
    out[0, 1:-1, 1:-1] = np.where(red_row, mine, other)
    out[1, 1:-1, 1:-1] = green
    out[2, 1:-1, 1:-1] = np.where(red_row, other, mine)
    out[:, :, 0] = out[:, :, 1]
    out[:, :, W - 1] = out[:, :, W - 2]
    out[:, 0, :] = out[:, 1, :]
    out[:, H - 1, :] = out[:, H - 2, :]
    return out.astype(np.uint8)


def demosaic_scalar(raw: np.ndarray, pattern: str) -> np.ndarray:
    """The same, site by site as the definition reads (tests hold `demosaic` to it)."""
    H, W = raw.shape
    assert H >= 3 and W >= 3
    ry, rx = BAYER[pattern]
    r = raw.astype(np.int32)
    out = np.zeros((3, H, W), dtype=np.int32)
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            c = r[y, x]
            cross = r[y - 1, x] + r[y + 1, x] + r[y, x - 1] + r[y, x + 1]
            diag = r[y - 1, x - 1] + r[y - 1, x + 1] + r[y + 1, x - 1] + r[y + 1, x + 1]
            red_row = (y & 1) == ry
            if ((x & 1) == rx) == red_row:           # an R site (in a red row) or a B site (in a blue row)
                own, opp = (0, 2) if red_row else (2, 0)
                out[own, y, x] = c
                out[1, y, x] = (cross + 2) >> 2
                out[opp, y, x] = (diag + 2) >> 2
            else:                                    # a G site: its row's colour left and right, the other above and below
                hor, ver = (0, 2) if red_row else (2, 0)
                out[1, y, x] = c
                out[hor, y, x] = (r[y, x - 1] + r[y, x + 1] + 1) >> 1
                out[ver, y, x] = (r[y - 1, x] + r[y + 1, x] + 1) >> 1
    out[:, :, 0] = out[:, :, 1]
    out[:, :, W - 1] = out[:, :, W - 2]
    out[:, 0, :] = out[:, 1, :]
    out[:, H - 1, :] = out[:, H - 2, :]
    return out.astype(np.uint8)


def unpack(buf, encoding: str, H: int, W: int, step=None, bgr: bool = False, channels=None) -> np.ndarray:
    """One frame -> uint8 [C,H,W] planar: C = 1 for mono8 (3 when asked for: the plane replicated), 3 otherwise (R,G,B; `bgr`: B,G,R)."""
    if encoding not in ENCODINGS:
        raise ValueError(f"unknown encoding {encoding!r}")
    rows = rows_of(buf, encoding, H, W, step)
    if encoding == "mono8":
        return np.repeat(rows[None], 3 if channels == 3 else 1, axis=0)
    if encoding == "planar":
        rgb = rows.reshape(3, H, W)
    elif encoding in BAYER:
        rgb = demosaic(rows, encoding)
    else:
        rgb = rows.reshape(H, W, 3).transpose(2, 0, 1)
        if encoding == "bgr8":
            rgb = rgb[::-1]
    return np.ascontiguousarray(rgb[::-1] if bgr else rgb)


# ---------------------------------------------------------------------------------------------------------------------- map
def default_new_K(K, src_size, out_size) -> np.ndarray:
    """image_proc's P = K, scaled to the output size by the width and height ratios."""
    (H, W), (h, w) = src_size, out_size
    return np.diag([w / W, h / H, 1.0]) @ np.asarray(K, dtype=np.float64).reshape(3, 3)


def rectify_map(K, D, model: str, src_size, out_size=None, new_K=None, R=None):
    """(qx, qy): int32 [h,w] Q5 source coordinates of every output pixel."""
    H, W = src_size
    h, w = src_size if out_size is None else out_size
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kn = default_new_K(K, (H, W), (h, w)) if new_K is None else np.asarray(new_K, dtype=np.float64).reshape(3, 3)
    Rt = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3).T
    D = [float(d) for d in D]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        M = Rt @ np.linalg.inv(Kn)
        X, Y, Z = (M[i, 0] * u + M[i, 1] * v + M[i, 2] for i in range(3))
        x, y = X / Z, Y / Z
        if model == "plumb_bob":
            k1, k2, p1, p2, k3 = D if len(D) == 5 else D + [0.0]
            r2 = x * x + y * y
            rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        elif model == "equidistant":
            k1, k2, k3, k4 = D
            r = np.sqrt(x * x + y * y)
            t = np.arctan(r)
            t2 = t * t
            td = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r == 0, 1.0, td / np.where(r == 0, 1.0, r))
            xd, yd = x * s, y * s
        else:
            raise ValueError(f"unknown distortion model {model!r}")
        sx = K[0, 0] * xd + K[0, 2]
        sy = K[1, 1] * yd + K[1, 2]
        sx = np.clip(np.where(np.isfinite(sx), sx, SENTINEL), -2, W + 1)
        sy = np.clip(np.where(np.isfinite(sy), sy, SENTINEL), -2, H + 1)
    qx = np.rint(Q * sx).astype(np.int32).reshape(h, w)
    qy = np.rint(Q * sy).astype(np.int32).reshape(h, w)
    return qx, qy


def map_point(K, D, model, src_size, Kn, R, u, v):
    """The same map for ONE output pixel in plain `math` (an independent statement for tests): (qx, qy)."""
    H, W = src_size
    Ki = np.linalg.inv(np.asarray(Kn, dtype=np.float64).reshape(3, 3))
    Rt = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3).T
    M = Rt @ Ki
    X, Y, Z = (M[i, 0] * u + M[i, 1] * v + M[i, 2] for i in range(3))
    x, y = X / Z, Y / Z
    if model == "plumb_bob":
        k1, k2, p1, p2 = D[:4]
        k3 = D[4] if len(D) > 4 else 0.0
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    else:
        r = math.sqrt(x * x + y * y)
        t = math.atan(r)
        td = t * (1 + t ** 2 * (D[0] + t ** 2 * (D[1] + t ** 2 * (D[2] + t ** 2 * D[3]))))
        s = td / r if r else 1.0
        xd, yd = x * s, y * s
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    out = []
    for c, lim in ((K[0, 0] * xd + K[0, 2], W + 1), (K[1, 1] * yd + K[1, 2], H + 1)):
        c = float(c)
        c = float(SENTINEL) if not math.isfinite(c) else min(max(c, -2.0), float(lim))
        out.append(int(round(Q * c)))   # Python's round: ties to even, like rint
    return tuple(out)


def tap_classes(qx, qy, H: int, W: int):
    """(full, partial, none): boolean [h,w] masks -- all four taps inside the H x W frame, some of them, none."""
    ix, iy = qx >> 5, qy >> 5
    inx = [(ix + d >= 0) & (ix + d <= W - 1) for d in (0, 1)]
    iny = [(iy + d >= 0) & (iy + d <= H - 1) for d in (0, 1)]
    n = sum((a & b).astype(int) for a in inx for b in iny)
    return n == 4, (n > 0) & (n < 4), n == 0


# ----------------------------------------------------------------------------------------------------------------- sampling
def sample(planes: np.ndarray, qx: np.ndarray, qy: np.ndarray) -> np.ndarray:
    """uint8 [C,H,W] sampled at the Q5 map -> uint8 [C,h,w]."""
    C, H, W = planes.shape
    pad = np.zeros((C, H + 2, W + 2), dtype=np.int64)   # index i + 1 holds pixel i; -1 and H (W) are the zero border
    pad[:, 1:-1, 1:-1] = planes
    ix, iy = (qx >> 5).astype(np.int64), (qy >> 5).astype(np.int64)
    ax, ay = (qx & 31).astype(np.int64), (qy & 31).astype(np.int64)

    def tap(dy, dx):
        yy, xx = iy + dy, ix + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok, pad[:, np.clip(yy, -1, H) + 1, np.clip(xx, -1, W) + 1], 0)

    acc = (32 - ax) * (32 - ay) * tap(0, 0) + ax * (32 - ay) * tap(0, 1) + (32 - ax) * ay * tap(1, 0) + ax * ay * tap(1, 1)
    return ((acc + 512) >> 10).astype(np.uint8)


def rectify(buf, encoding: str, H: int, W: int, qx, qy, step=None, bgr: bool = False, channels=None) -> np.ndarray:
    """One frame of any source kind -> uint8 [C,h,w]: unpack (demosaic included), then sample."""
    return sample(unpack(buf, encoding, H, W, step, bgr, channels), qx, qy)
