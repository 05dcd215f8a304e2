"""Write tests/golden/jpeg_cases.pt: the byte streams of the JPEG ingest tests (needs Pillow; the tests that read the file do not).

    python scripts/make_jpeg_fixtures.py

Streams only: the expected pixels come from tests/jpeg_ref.py at run time.  Pictures are crops of tests/golden/demo_frames_raw.pt
and seeded noise (noise at high quality reaches the large coefficients a photograph never has).  Every case is
{"name", "data": bytes, "status": name of the expected WVN_JPEG_* status, "sampling", "size": (W, H)}.
"""
import io
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_cases.pt")

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 23), (33, 47)]          # (W, H)
SAMPLINGS = {"gray": None, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2}          # Pillow's `subsampling`


def picture(demo, rng, W, H, kind):
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    y0, x0 = int(rng.integers(0, demo.shape[0] - H + 1)), int(rng.integers(0, demo.shape[1] - W + 1))
    return demo[y0:y0 + H, x0:x0 + W]


def encode(rgb, sampling, quality, **kw):
    im = Image.fromarray(rgb)
    if sampling == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = SAMPLINGS[sampling]
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def find(data, marker, start=0):
    """Offset of the first segment `marker` (walks the segments: no false hit inside a payload)."""
    p = 2
    while p < len(data):
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == marker and p >= start:
            return p
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    raise KeyError(marker)


def widen_dqt(data):
    """Every DQT rewritten with 16-bit entries (Pq = 1), every entry multiplied by 9: tables beyond 255, which Pillow's encoder cannot
    write (it clamps `qtables` to the baseline range).  The decoded picture has 9 times the contrast."""
    out, p = bytearray(data[:2]), 2
    while True:
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + n]
        if m == 0xDB:
            body, q = bytearray(), 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                body.append(0x10 | (seg[q] & 15))
                for k, v in enumerate(seg[q + 1:q + 65]):
                    body += int(v * 9).to_bytes(2, "big")
                q += 65
            out += b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
        else:
            out += data[p:p + 2 + n]
        p += 2 + n
        if m == 0xDA:
            return bytes(out + data[p:])


def main():
    demo_all = torch.load(os.path.join(ROOT, "tests", "golden", "demo_frames_raw.pt"), weights_only=False)["frames_u8"]
    demo = demo_all[1].permute(1, 2, 0).contiguous().numpy()             # [224, 299, 3]
    rng = np.random.default_rng(20240607)
    cases = []

    def add(name, data, sampling, size, status="OK"):
        cases.append({"name": name, "data": bytes(data), "status": status, "sampling": sampling, "size": tuple(size)})

    for i, (W, H) in enumerate(SIZES):
        for sampling in SAMPLINGS:
            rgb = picture(demo, rng, W, H, "noise" if i % 2 == 0 else "demo")
            add(f"{W}x{H}_{sampling}_q75", encode(rgb, sampling, 75), sampling, (W, H))
    for W, H in ((17, 23), (33, 47)):
        for sampling in SAMPLINGS:
            for q, kind in ((30, "demo"), (95, "noise"), (100, "noise")):
                add(f"{W}x{H}_{sampling}_q{q}", encode(picture(demo, rng, W, H, kind), sampling, q), sampling, (W, H))
            add(f"{W}x{H}_{sampling}_optimize", encode(picture(demo, rng, W, H, "demo"), sampling, 85, optimize=True), sampling, (W, H))
            add(f"{W}x{H}_{sampling}_rst_blocks1", encode(picture(demo, rng, W, H, "noise"), sampling, 80, restart_marker_blocks=1),
                sampling, (W, H))
            add(f"{W}x{H}_{sampling}_rst_rows1", encode(picture(demo, rng, W, H, "demo"), sampling, 80, restart_marker_rows=1),
                sampling, (W, H))
    # custom quantisation tables, and the same streams with 16-bit DQT entries beyond 255
    custom = [[min(1 + 4 * k, 255) for k in range(64)], [min(3 + 5 * k, 255) for k in range(64)]]
    for sampling in ("gray", "4:4:4", "4:2:0"):
        rgb = picture(demo, rng, 33, 47, "demo")
        data = encode(rgb, sampling, 75, qtables=custom[:1] if sampling == "gray" else custom)
        add(f"33x47_{sampling}_qt8", data, sampling, (33, 47))
        # a picture of a ninth of the contrast, so that the widened tables give back a picture of 8-bit samples ...
        faint = (128 + (rgb.astype(np.int32) - 128) // 9).astype(np.uint8)
        data = encode(faint, sampling, 75, qtables=custom[:1] if sampling == "gray" else custom)
        add(f"33x47_{sampling}_qt16", widen_dqt(data), sampling, (33, 47))
    # ... and the full-contrast one, which then leaves the range in which libjpeg has one answer
    add("out_of_range_qt16", widen_dqt(encode(picture(demo, rng, 33, 47, "noise"), "4:2:0", 75, qtables=custom)), None, (33, 47), "OUT_OF_RANGE")
    for sampling in SAMPLINGS:
        add(f"299x224_{sampling}_q75", encode(demo, sampling, 75), sampling, (299, 224))
    add("299x224_4:2:0_q30", encode(demo, "4:2:0", 30), "4:2:0", (299, 224))
    add("299x224_4:2:0_q95", encode(demo, "4:2:0", 95), "4:2:0", (299, 224))
    # a one-component file whose sampling factors are 2x2: they mean nothing in a scan that is not interleaved
    g = bytearray(encode(picture(demo, rng, 17, 23, "demo"), "gray", 75))
    sof = find(g, 0xC0)
    assert g[sof + 11] == 0x11
    g[sof + 11] = 0x22
    add("17x23_gray_factors2x2", g, "gray", (17, 23))

    # ---- refusals and corruptions of one valid stream
    base = encode(picture(demo, rng, 33, 47, "demo"), "4:2:0", 75)
    add("refuse_progressive", encode(picture(demo, rng, 33, 47, "demo"), "4:2:0", 75, progressive=True), None, (33, 47), "UNSUPPORTED")
    buf = io.BytesIO()
    Image.fromarray(picture(demo, rng, 33, 47, "demo")).convert("CMYK").save(buf, "JPEG", quality=75)
    add("refuse_cmyk", buf.getvalue(), None, (33, 47), "UNSUPPORTED")
    add("refuse_4:4:0", encode(picture(demo, rng, 33, 47, "demo"), "4:4:4", 75).replace(b"\x01\x11\x00\x02\x11", b"\x01\x12\x00\x02\x11", 1),
        None, (33, 47), "UNSUPPORTED")
    sos = find(base, 0xDA)
    scan = sos + 2 + ((base[sos + 2] << 8) | base[sos + 3])
    dht = find(base, 0xC4)
    add("truncated_at_marker", base[:sos], None, (33, 47), "TRUNCATED")
    add("truncated_in_table", base[:dht + 30], None, (33, 47), "TRUNCATED")
    add("truncated_mid_scan", base[:scan + (len(base) - scan) // 2], None, (33, 47), "TRUNCATED")
    add("truncated_no_eoi", base[:-2], None, (33, 47), "TRUNCATED")
    bad = bytearray(base)
    bad[scan:scan + 4] = b"\xff\x00\xff\x00"          # sixteen 1 bits: no code of the standard DC table
    add("bad_huffman", bad, None, (33, 47), "BAD_HUFFMAN")
    bad = bytearray(base)
    bad[dht + 4] = 0x13                               # the first DHT now defines AC table 3: DC table 0, which the scan names, is never defined
    add("bad_table_missing", bad, None, (33, 47), "BAD_TABLE")
    add("not_a_jpeg", b"\x89PNG\r\n\x1a\n" + bytes(24), None, (0, 0), "BAD_MARKER")

    import jpeg_ref

    for c in cases:   # the file is only written if the definition agrees with the intent of every case
        try:
            jpeg_ref.decode(c["data"])
            got = "OK"
        except jpeg_ref.JpegError as e:
            got = e.args[0]
        assert got == c["status"], (c["name"], got, c["status"])
    torch.save({"cases": cases, "pillow": Image.__version__ if hasattr(Image, "__version__") else ""}, OUT)
    print(f"{len(cases)} cases, {sum(len(c['data']) for c in cases)} bytes of streams -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
