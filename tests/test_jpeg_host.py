"""JPEG ingest without a GPU: tests/jpeg_ref.py (the definition) against Pillow at zero differing bytes, the library's host stage
(parser + Huffman decoder, csrc/jpeg_host.cpp) against jpeg_ref coefficient for coefficient, the status of every refusal and
corruption, and the stand-alone sanitizer run of the parser over a few thousand mutants (tests/jpeg_fuzz_main.cpp)."""
import ctypes as C
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(golden):
    return golden("jpeg_cases.pt")["cases"]


def _valid(cases):
    return [c for c in cases if c["status"] == "OK"]


def _pillow_rgb(data):
    from PIL import Image      # a hard requirement of this file: without Pillow the definition is not pinned, and that is a failure

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).transpose(2, 0, 1)


# ------------------------------------------------------------------------------------------------ the definition against Pillow
def test_fixture_file_covers_the_issue_table(cases):
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for W, H in ((1, 1), (7, 5), (8, 8), (16, 16), (17, 23), (33, 47), (299, 224)):
        for s in ("gray", "4:4:4", "4:2:2", "4:2:0"):
            assert any(c["size"] == (W, H) and c["sampling"] == s and c["status"] == "OK" for c in cases), (W, H, s)
    for tag in ("_q30", "_q75", "_q95", "_q100", "_optimize", "_qt16", "_rst_blocks1", "_rst_rows1"):
        assert any(tag in n for n in names), tag
    assert max(len(c["data"]) for c in cases) < 64 * 1024
    # the 16-bit DQT is really there, and so are the restart markers
    wide = next(c for c in cases if c["name"] == "33x47_4:2:0_qt16")
    assert max(t.max() for t in jpeg_ref.parse(wide["data"]).qt.values()) > 255
    assert jpeg_ref.parse(next(c for c in cases if c["name"] == "33x47_4:2:0_rst_blocks1")["data"]).restart == 1


def test_ref_equals_pillow_on_every_fixture(cases):
    for c in _valid(cases):
        want = _pillow_rgb(c["data"])
        got = jpeg_ref.decode(c["data"])
        assert got.shape == want.shape and got.dtype == np.uint8, c["name"]
        assert int((got != want).sum()) == 0, c["name"]


def test_ref_equals_pillow_on_fresh_random_streams():
    from PIL import Image

    rng = np.random.default_rng(7)
    n = 0
    for it in range(200):
        W, H = (int(v) for v in rng.integers(1, 70, 2))
        if it % 10 == 0:
            W = int(rng.integers(1, 6))      # the widths at which libjpeg replaces fancy upsampling by replication
        q = int(rng.choice([1, 10, 30, 50, 75, 90, 95, 100]))
        kind = it % 3
        if kind == 0:
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif kind == 1:   # smooth ramps: low-frequency coefficients only
            a = (np.add.outer(np.arange(H) * 3, np.arange(W) * 5)[..., None] * np.array([1, 2, 3]) % 256).astype(np.uint8)
        else:             # saturated checkers: the range limits
            a = (((np.add.outer(np.arange(H) // 3, np.arange(W) // 2) % 2) * 255)[..., None] * np.array([1, 0, 1]) +
                 np.array([0, 255, 0]) * (it % 2)).astype(np.uint8)
        im = Image.fromarray(a)
        kw = {}
        sub = (None, 0, 1, 2)[(it // 3) % 4]
        if sub is None:
            im = im.convert("L")
        else:
            kw["subsampling"] = sub
        if it % 7 == 0:
            kw["optimize"] = True
        if it % 11 == 0:
            kw["restart_marker_blocks"] = int(rng.integers(1, 5))
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=q, **kw)
        data = buf.getvalue()
        assert int((jpeg_ref.decode(data) != _pillow_rgb(data)).sum()) == 0, (it, W, H, q, sub, kw)
        n += 1
    assert n == 200


# ------------------------------------------------------------------------------------------------ the library's host stage
def test_abi_is_registered():
    for name in ("wvn_jpeg_info", "wvn_jpeg_probe_batch", "wvn_jpeg_coef_bytes", "wvn_jpeg_plane_bytes", "wvn_jpeg_workspace_bytes", "wvn_jpeg_coefficients",
                 "wvn_jpeg_decode_batch"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert C.sizeof(_lib.JpegGeometry) == 20
    h = _lib.lib()
    g = _lib.JpegGeometry(448, 448, 3, 3, 0)
    # 4:2:0 at 448 x 448: 4704 blocks of 128 B = the bytes of the RGB8 frame
    assert h.wvn_jpeg_coef_bytes(C.byref(g)) == 4704 * 128 == 448 * 448 * 3
    assert h.wvn_jpeg_plane_bytes(C.byref(g)) == 4704 * 64
    assert h.wvn_jpeg_workspace_bytes(C.byref(g), 2) >= 2 * (512 + 4704 * 192)
    for bad in (_lib.JpegGeometry(0, 8, 3, 3, 0), _lib.JpegGeometry(8, 8, 1, 3, 0), _lib.JpegGeometry(8, 8, 3, 7, 0),
                _lib.JpegGeometry(8, 20000, 3, 3, 0)):
        assert h.wvn_jpeg_coef_bytes(C.byref(bad)) == 0 and h.wvn_jpeg_workspace_bytes(C.byref(bad), 1) == 0
    # refused before anything is touched or launched: no GPU needed
    one = (C.c_void_p * 1)(1 << 20)
    n = (C.c_size_t * 1)(16)
    st = (C.c_int * 1)()
    assert h.wvn_jpeg_decode_batch(one, n, 0, C.byref(g), 1 << 20, 0, 1 << 20, 8, st, None) == 1001
    assert h.wvn_jpeg_decode_batch(one, n, 1, C.byref(g), 1 << 20, 1, 1 << 20, 8, st, None) == 1001     # gray_out on a colour geometry
    assert h.wvn_jpeg_decode_batch(one, n, 1, C.byref(g), None, 0, 1 << 20, 8, st, None) == 1001


def test_info(cases):
    for c in _valid(cases):
        i = ops.jpeg_info(c["data"])
        assert (i["width"], i["height"]) == c["size"] and i["sampling"] == c["sampling"], c["name"]
        assert i["components"] == (1 if c["sampling"] == "gray" else 3)
        assert i["restart_interval"] == jpeg_ref.parse(c["data"]).restart
    assert ops.jpeg_info(bytearray(_valid(cases)[0]["data"]))["width"] == 1
    assert ops.jpeg_info(torch.frombuffer(bytearray(_valid(cases)[5]["data"]), dtype=torch.uint8))["width"] == 7


def test_coefficients_equal_the_reference(cases):
    for c in _valid(cases):
        f, want, want_qt = jpeg_ref.coefficients_flat(c["data"])
        rc, coef, qt, g = ops.jpeg_coefficients(c["data"])
        assert rc == 0, c["name"]
        assert coef.shape == want.shape and np.array_equal(coef.numpy(), want), c["name"]
        assert np.array_equal(qt.numpy(), want_qt.astype(np.int32)), c["name"]


def test_status_of_every_refusal_and_corruption(cases):
    bad = [c for c in cases if c["status"] != "OK"]
    assert {c["status"] for c in bad} >= {"UNSUPPORTED", "TRUNCATED", "BAD_HUFFMAN", "BAD_TABLE", "BAD_MARKER"}
    g = _lib.JpegGeometry(33, 47, 3, 3, 0)
    nbytes = _lib.lib().wvn_jpeg_coef_bytes(C.byref(g))
    for c in bad:
        want = _lib.JPEG_STATUS.index(c["status"])
        a = np.frombuffer(c["data"], dtype=np.uint8)
        # wvn_jpeg_info walks the header; what it lets through fails in the scan, with arrays sized for the frame it announced
        coef = torch.full((nbytes // 2,), 7, dtype=torch.int16)
        qt = torch.full((192,), 7, dtype=torch.int16)
        rc = _lib.lib().wvn_jpeg_coefficients(a.ctypes.data, a.size, C.byref(g), coef.data_ptr(), nbytes, qt.data_ptr())
        assert rc == want, (c["name"], rc)
        assert int(coef.abs().sum()) == 0 and int(qt.abs().sum()) == 0, c["name"]      # a failed frame leaves nothing behind
        gi = _lib.JpegGeometry()
        rci = _lib.lib().wvn_jpeg_info(a.ctypes.data, a.size, C.byref(gi))
        assert rci in (0, want), c["name"]
        with pytest.raises(_lib.WvnError, match="WVN_JPEG_" + c["status"]) if rci else _noraise():
            ops.jpeg_info(c["data"])
    # a valid frame of another geometry than the arrays were sized for
    other = next(c for c in cases if c["name"] == "17x23_4:2:0_q75")
    a = np.frombuffer(other["data"], dtype=np.uint8)
    coef = torch.zeros(nbytes // 2, dtype=torch.int16)
    qt = torch.zeros(192, dtype=torch.int16)
    assert _lib.lib().wvn_jpeg_coefficients(a.ctypes.data, a.size, C.byref(g), coef.data_ptr(), nbytes, qt.data_ptr()) == _lib.JPEG_GEOMETRY_MISMATCH
    assert _lib.lib().wvn_jpeg_coefficients(a.ctypes.data, a.size, C.byref(g), coef.data_ptr(), nbytes - 2, qt.data_ptr()) == 1002


class _noraise:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_every_truncation_of_a_stream_is_a_status(cases):
    """No prefix of a valid stream decodes, and none reads past its end (the sanitizer run below watches the same walk)."""
    c = next(c for c in cases if c["name"] == "17x23_4:2:0_rst_blocks1")
    data = c["data"]
    g = _lib.JpegGeometry(17, 23, 3, 3, 1)
    nbytes = _lib.lib().wvn_jpeg_coef_bytes(C.byref(g))
    coef = torch.zeros(nbytes // 2, dtype=torch.int16)
    qt = torch.zeros(192, dtype=torch.int16)
    seen = set()
    for n in range(1, len(data)):
        a = np.frombuffer(data[:n], dtype=np.uint8).copy()
        rc = _lib.lib().wvn_jpeg_coefficients(a.ctypes.data, a.size, C.byref(g), coef.data_ptr(), nbytes, qt.data_ptr())
        assert rc != 0, n
        seen.add(rc)
    assert _lib.JPEG_TRUNCATED in seen and seen <= {_lib.JPEG_TRUNCATED, _lib.JPEG_BAD_MARKER}, seen


def _c_status(data, g=None):
    """Status of the library's host stage for one stream, decoded as a member of a batch of geometry g (default: its own)."""
    h = _lib.lib()
    a = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    n = len(data)
    if g is None:
        g = _lib.JpegGeometry()
        rc = h.wvn_jpeg_info(a.ctypes.data, n, C.byref(g))
        if rc:
            return rc
    nbytes = h.wvn_jpeg_coef_bytes(C.byref(g))
    coef = torch.empty(nbytes // 2, dtype=torch.int16)
    qt = torch.empty(192, dtype=torch.int16)
    return h.wvn_jpeg_coefficients(a.ctypes.data, n, C.byref(g), coef.data_ptr(), nbytes, qt.data_ptr())


def _ref_status(data):
    try:
        jpeg_ref.decode(data)
        return 0
    except jpeg_ref.JpegError as e:
        return jpeg_ref.STATUS.index(e.args[0])


def _scan_start(data):
    p = 2
    while True:
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        p += 2 + n
        if m == 0xDA:
            return p


def test_bytes_left_in_front_of_a_marker_are_refused(cases):
    """libjpeg skips "extraneous bytes before marker"; here 1 to 12 bytes of junk between the last coded bit and EOI or RSTn are
    WVN_JPEG_BAD_MARKER, however many of them the bit reader had already fetched."""
    base = next(c for c in cases if c["name"] == "33x47_4:2:0_q75")["data"]
    rst = next(c for c in cases if c["name"] == "33x47_4:2:0_rst_blocks1")["data"]
    assert _c_status(base) == 0 and _c_status(rst) == 0
    first_rst = rst.index(b"\xff\xd0", _scan_start(rst))
    last_rst = max(i for i in range(first_rst, len(rst) - 1) if rst[i] == 0xFF and 0xD0 <= rst[i + 1] <= 0xD7)
    assert last_rst > first_rst
    for k in (1, 2, 3, 5, 7, 8, 9, 12):
        junk = bytes([0x5A, 0x13, 0x00, 0x7F] * 3)[:k]
        for name, bad in (("EOI", base[:-2] + junk + base[-2:]), ("first RSTn", rst[:first_rst] + junk + rst[first_rst:]),
                          ("last RSTn", rst[:last_rst] + junk + rst[last_rst:]), ("EOI behind restarts", rst[:-2] + junk + rst[-2:])):
            assert _ref_status(bad) == _lib.JPEG_BAD_MARKER, (name, k)
            assert _c_status(bad) == _lib.JPEG_BAD_MARKER, (name, k)


def test_status_equals_the_reference_on_seeded_mutants(cases):
    """The library's host stage and tests/jpeg_ref.py give every stream the same status: 1500 seeded mutants (one byte replaced, one
    byte inserted, or cut short) of the streams below 1.5 KB, each decoded as itself and, where its header no longer reads, as a
    member of a batch of its origin's geometry.  The first error in stream order decides; OUT_OF_RANGE comes last in both."""
    rng = np.random.default_rng(11)
    small = [c for c in cases if len(c["data"]) < 1500 and c["size"] != (0, 0)]
    assert len(small) >= 40
    seen, n = {}, 0
    for it in range(1500):
        c = small[it % len(small)]
        d = bytearray(c["data"])
        kind = it % 4
        start = _scan_start(c["data"]) if c["status"] == "OK" and it % 3 else 0      # two thirds inside the entropy-coded data
        start = min(start, len(d) - 1)
        pos = int(rng.integers(start, len(d)))
        if kind == 0:
            d = d[:pos]
        elif kind == 1:
            d.insert(pos, int(rng.integers(0, 256)))
        else:
            d[pos] = int(rng.integers(0, 256))
        d = bytes(d)
        want = _ref_status(d)
        got = _c_status(d) if len(d) else _lib.JPEG_TRUNCATED
        assert got == want, (c["name"], it, kind, pos, _lib.JPEG_STATUS[got], jpeg_ref.STATUS[want])
        seen[want] = seen.get(want, 0) + 1
        n += 1
    assert n == 1500 and seen.get(0, 0) > 50 and len(seen) >= 6, seen      # mutants that still decode, and six kinds of refusal


def _host_batch(group, g, threads):
    h = _lib.lib()
    B = len(group)
    bufs = [np.frombuffer(c["data"], dtype=np.uint8) for c in group]
    one = h.wvn_jpeg_coef_bytes(C.byref(g))
    coef = torch.full((B, one // 128, 64), -3, dtype=torch.int16)
    qt = torch.full((B, 3, 64), -3, dtype=torch.int16)
    status = (C.c_int * B)(*([99] * B))
    rc = h.wvn_jpeg_coefficients_batch((C.c_void_p * B)(*[a.ctypes.data for a in bufs]), (C.c_size_t * B)(*[a.size for a in bufs]), B,
                                       C.byref(g), coef.data_ptr(), B * one, qt.data_ptr(), threads, status)
    assert rc == 0
    return coef, qt, list(status)


def test_threads_do_not_change_the_output(cases):
    """The host stage of a batch (wvn_jpeg_coefficients_batch: the worker pool of wvn_jpeg_decode_batch without the device) on 1 and
    on 8 workers, a corrupt and a foreign member included: same arrays, same statuses, and each frame equals its single decode."""
    group = [c for c in cases if c["size"] == (33, 47) and c["sampling"] in ("4:2:0", None)]
    group.append(next(c for c in cases if c["name"] == "17x23_4:2:0_q75"))
    assert len(group) >= 12 and sum(c["status"] != "OK" for c in group) >= 5
    g = _lib.JpegGeometry(33, 47, 3, 3, 0)
    c1, q1, s1 = _host_batch(group, g, 1)
    for threads in (8, 16, 1000, 0):        # (above the cap of 16 and below 1: clamped, never sized from the machine)
        c8, q8, s8 = _host_batch(group, g, threads)
        assert torch.equal(c1, c8) and torch.equal(q1, q8) and s1 == s8, threads
    for i, c in enumerate(group):
        want = _lib.JPEG_GEOMETRY_MISMATCH if c["name"].startswith("17x23") else _lib.JPEG_STATUS.index(c["status"])
        assert s1[i] == want, c["name"]
        if want == 0:
            assert np.array_equal(c1[i].numpy(), jpeg_ref.coefficients_flat(c["data"])[1]), c["name"]
        else:
            assert int(c1[i].abs().sum()) == 0 and int(q1[i].abs().sum()) == 0, c["name"]


def test_mixed_geometry_and_bad_arguments_are_refused_in_python(cases):
    a = next(c for c in cases if c["name"] == "17x23_4:2:0_q75")["data"]
    b = next(c for c in cases if c["name"] == "33x47_4:2:0_q75")["data"]
    c = next(c for c in cases if c["name"] == "17x23_4:2:2_q75")["data"]
    # (geometry is checked before the device: a fake GPU ordinal is never touched)
    for pair in ((a, b), (a, c)):
        with pytest.raises(_lib.WvnError, match="mixed geometry"):
            ops.jpeg_decode(list(pair), "cuda:0", strict=False)
    with pytest.raises(_lib.WvnError, match="no CPU fallback"):
        ops.jpeg_decode(a, "cpu")
    for threads in (0, 17, os.cpu_count() + 17):
        with pytest.raises(_lib.WvnError, match="threads"):
            ops.jpeg_decode(a, "cuda:0", threads=threads)
    with pytest.raises(_lib.WvnError, match="gray=True"):
        ops.jpeg_decode(a, "cuda:0", gray=True)
    with pytest.raises(_lib.WvnError, match="frame 1: WVN_JPEG_TRUNCATED"):
        ops.jpeg_decode([a, a[:200]], "cuda:0")
    with pytest.raises(_lib.WvnError):
        ops.jpeg_decode([], "cuda:0")
    with pytest.raises(_lib.WvnError):
        ops.jpeg_decode([a, "not bytes"], "cuda:0")


# ------------------------------------------------------------------------------------------------ sanitizer run of the parser
def test_fuzz_program_runs_clean_under_the_sanitizers(cases, tmp_path):
    """tests/jpeg_fuzz_main.cpp + csrc/jpeg_host.cpp, built with the host compiler and -fsanitize=address,undefined, over every
    fixture and seeded single-byte and truncation mutants of them.  A stand-alone program: nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (g++ / clang++ / c++): the sanitizer run of the parser cannot be skipped"
    exe = tmp_path / "jpeg_fuzz"
    src = [os.path.join(ROOT, "tests", "jpeg_fuzz_main.cpp"), os.path.join(ROOT, "wild_visual_navigation_amd", "csrc", "jpeg_host.cpp")]
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                        "-o", str(exe)] + src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    corpus = tmp_path / "corpus.bin"
    with open(corpus, "wb") as f:       # [u32 count] then [u32 length, bytes] per stream
        f.write(np.uint32(len(cases)).tobytes())
        for c in cases:
            f.write(np.uint32(len(c["data"])).tobytes())
            f.write(c["data"])
    r = subprocess.run([str(exe), str(corpus), "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("jpeg_fuzz: ok"), line
    runs = int(line.split()[2])
    assert runs >= len(cases) * 40
