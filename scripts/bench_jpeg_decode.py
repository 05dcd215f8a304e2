"""JPEG ingest: ops.jpeg_decode against the route a user had before it -- Pillow in a 16-thread pool decoding into a reused pinned buffer, then one uint8 upload.

    python scripts/bench_jpeg_decode.py [--reps 20] [--out profiles/jpeg_decode.json]

Two shapes: 64 frames of 448 x 448 and 16 frames of 1440 x 1080 (the camera's size), 4:2:0, quality 90, pictures made from
tests/golden/demo_frames_raw.pt (resampled, shifted, a little sensor noise) so that the entropy-coded data is that of photographs.
Per frame: the host stage (parser + Huffman, wvn_jpeg_coefficients_batch), the upload of the coefficients from pinned memory, the
device stage (wvn_jpeg_device_stage: two kernels, device events) and the whole call (host clock around ops.jpeg_decode + synchronise);
the two routes alternate in the timed loop.  The device stage is also given as bytes it must move over its time.  Needs Pillow and a GPU.
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wild_visual_navigation_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12   # B/s, MI355X specification


def make_streams(B, W, H, quality=90):
    from PIL import Image

    demo = torch.load(os.path.join(ROOT, "tests", "golden", "demo_frames_raw.pt"), weights_only=False)["frames_u8"].float()
    rng = np.random.default_rng(5)
    out = []
    for b in range(B):
        src = demo[b % demo.shape[0]][None]
        big = torch.nn.functional.interpolate(src, size=(H + 32, W + 32), mode="bilinear", align_corners=False)[0]
        dy, dx = int(rng.integers(0, 33)), int(rng.integers(0, 33))
        a = big[:, dy:dy + H, dx:dx + W].permute(1, 2, 0).numpy()
        a = np.clip(a + rng.normal(0, 2.0, a.shape), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality, subsampling=2)
        out.append(buf.getvalue())
    return out


def median(v):
    return float(np.median(v))


def bench_shape(dev, B, W, H, reps, warmup=3):
    from PIL import Image

    streams = make_streams(B, W, H)
    h = _lib.lib()
    bufs = [np.frombuffer(s, dtype=np.uint8) for s in streams]
    ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in bufs])
    sizes = (C.c_size_t * B)(*[a.size for a in bufs])
    g = _lib.JpegGeometry()
    assert h.wvn_jpeg_info(bufs[0].ctypes.data, bufs[0].size, C.byref(g)) == 0
    one = h.wvn_jpeg_coef_bytes(C.byref(g))
    planes = h.wvn_jpeg_plane_bytes(C.byref(g))
    status = (C.c_int * B)()

    # -- the two routes must agree before anything is timed
    pool = ThreadPoolExecutor(16)

    # the yardstick decodes straight into ONE pinned buffer that is reused across calls, as a user of that route would
    pinned = torch.empty(B, H, W, 3, dtype=torch.uint8).pin_memory()
    pinned_np = pinned.numpy()

    def pillow_one(i):
        pinned_np[i] = np.asarray(Image.open(io.BytesIO(streams[i])).convert("RGB"))

    def pillow_route():
        list(pool.map(pillow_one, range(B)))
        return pinned.to(dev, non_blocking=True).permute(0, 3, 1, 2).contiguous()

    ours, st = ops.jpeg_decode(streams, dev, threads=16)
    assert st.abs().sum() == 0 and torch.equal(ours, pillow_route()), "the two routes disagree"

    # -- host stage alone, on 8 and on 16 workers
    coef = torch.empty(B * one // 2, dtype=torch.int16).pin_memory()
    qt = torch.empty(B * 192, dtype=torch.int16)
    host = {}
    for threads in (1, 8, 16):
        t = []
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            assert h.wvn_jpeg_coefficients_batch(ptrs, sizes, B, C.byref(g), coef.data_ptr(), B * one, qt.data_ptr(), threads, status) == 0
            t.append(time.perf_counter() - t0)
        host[threads] = median(t[warmup:]) / B
    # -- upload of the coefficients (pinned -> device), device events
    dcoef = torch.empty(B * one, dtype=torch.uint8, device=dev)
    src = coef.view(torch.uint8)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = []
    for r in range(warmup + reps):
        ev[0].record()
        dcoef.copy_(src, non_blocking=True)
        ev[1].record()
        ev[1].synchronize()
        t.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    upload = median(t[warmup:]) / B
    # -- device stage alone: the workspace of a real call, run again
    ws = torch.empty(h.wvn_jpeg_workspace_bytes(C.byref(g), B), dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, H, W, dtype=torch.uint8, device=dev)
    _lib.check(h.wvn_jpeg_decode_batch(ptrs, sizes, B, C.byref(g), out.data_ptr(), 0, ws.data_ptr(), 16, status, _lib.stream()), "decode")
    torch.cuda.synchronize()
    assert torch.equal(out, ours)
    t = []
    inner = 10
    for r in range(warmup + reps):
        ev[0].record()
        for _ in range(inner):
            _lib.check(h.wvn_jpeg_device_stage(C.byref(g), B, ws.data_ptr(), out.data_ptr(), 0, _lib.stream()), "device stage")
        ev[1].record()
        ev[1].synchronize()
        t.append(ev[0].elapsed_time(ev[1]) * 1e-3 / inner)
    device = median(t[warmup:]) / B
    assert torch.equal(out, ours)
    # bytes the device stage must move per frame: coefficients in, planes out; planes in, RGB out
    must_move = one + planes + planes + 3 * H * W
    # -- end to end, the two routes alternating
    e2e = {"ours_8": [], "ours_16": [], "pillow_16": []}
    for r in range(warmup + reps):
        for name in e2e:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "pillow_16":
                pillow_route()
            else:
                ops.jpeg_decode(streams, dev, threads=int(name.split("_")[1]))
            torch.cuda.synchronize()
            e2e[name].append(time.perf_counter() - t0)
    res = {
        "shape": f"{B} x {W}x{H}", "B": B, "W": W, "H": H, "stream_bytes_per_frame": int(np.mean([len(s) for s in streams])),
        "coef_bytes_per_frame": one, "rgb_bytes_per_frame": 3 * H * W,
        "host_us_per_frame": {str(k): v * 1e6 for k, v in host.items()},
        "upload_us_per_frame": upload * 1e6, "upload_GBps": one / upload / 1e9,
        "device_us_per_frame": device * 1e6, "device_must_move_bytes_per_frame": must_move,
        "device_achieved_TBps": must_move / device / 1e12, "device_share_of_hbm_peak": must_move / device / HBM_PEAK,
        "e2e_us_per_frame": {k: median(v[warmup:]) / B * 1e6 for k, v in e2e.items()},
        "e2e_spread_us_per_frame": {k: [min(v[warmup:]) / B * 1e6, max(v[warmup:]) / B * 1e6] for k, v in e2e.items()},
    }
    res["host_share_of_e2e_16"] = res["host_us_per_frame"]["16"] / res["e2e_us_per_frame"]["ours_16"]
    res["ratio_pillow_over_ours_16"] = res["e2e_us_per_frame"]["pillow_16"] / res["e2e_us_per_frame"]["ours_16"]
    pool.shutdown()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode: needs a GPU (a CPU run gives no time)")
    dev = torch.device("cuda:0")
    results = [bench_shape(dev, 64, 448, 448, a.reps), bench_shape(dev, 16, 1440, 1080, a.reps)]
    for r in results:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
