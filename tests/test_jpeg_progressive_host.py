"""No GPU: the marker walk of progressive files (maf-yolo_amd/jpeg.py parse(progressive=True)) and the restatement of libjpeg's progressive
Huffman decoder (tests/jpeg_progressive_ref.py).

* the restatement equals the fixture pixels (tests/golden/jpeg_progressive_cases.npz, written by tools/make_golden_jpeg_progressive.py with
  Pillow / libjpeg-turbo) exactly for every case, the 480 x 640 one by its sha256; where Pillow is importable also a fresh Pillow decode;
* over the fixture set every hard branch of jdphuff.c is taken (the restatement's counters);
* parse(progressive=True) gives the scans of libjpeg's jpeg_simple_progression, each with the Huffman tables and restart interval in force at
  its SOS; without the flag parse and supported still refuse;
* every unsupported progression raises JpegUnsupported naming it (header edits); truncation raises a plain MafError; a file whose LAST scan
  is cut short passes the parser (a short scan is the decoder's finding), a file that lacks a scan does not.
"""
import hashlib
import io

import numpy as np
import pytest

import jpeg_progressive_ref as P
from maf_yolo_amd import jpeg as J
from maf_yolo_amd.lib import MafError

# jcparam.c jpeg_simple_progression: (components, Ss, Se, Ah, Al); component 2 (Cr) goes before component 1 (Cb)
YCC_SCRIPT = [((0, 1, 2), 0, 0, 0, 1),
              ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
              ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0),
              ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
GRAY_SCRIPT = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


@pytest.fixture(scope="module")
def cases(golden):
    return golden("jpeg_progressive_cases")


def _names(z):
    return [str(n) for n in z["names"]]


def _sos(d):
    """Offsets of the 0xFF of every SOS marker, from the parser-independent fact that Pillow writes SOS segments of 6 + 2 n bytes."""
    info = J.parse(d, progressive=True)
    return [sc.range[0] - (8 + 2 * len(sc.components)) for sc in info.scans]


def _edit(d, at, value):
    b = bytearray(d)
    b[at] = value
    return bytes(b)


def test_restatement_equals_the_fixture_pixels_and_takes_every_branch(cases):
    P.reset_counters()
    for n in _names(cases):
        got = P.decode(cases["file_" + n].tobytes())
        want = cases["bgr_" + n]
        assert got.dtype == np.uint8 and got.shape == want.shape, n
        assert np.array_equal(got, want), n
    print(P.COUNTERS)
    for name in P.COUNTER_NAMES:
        assert P.COUNTERS[name] > 0, name


def test_restatement_large_case_sha256(cases):
    got = P.decode(cases["large_file"].tobytes())
    assert got.shape == (480, 640, 3)
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(cases["large_sha256"])


def test_restatement_equals_a_fresh_pillow_decode(cases):
    Image = pytest.importorskip("PIL.Image")
    for n in _names(cases):
        d = cases["file_" + n].tobytes()
        want = np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]
        assert np.array_equal(cases["bgr_" + n], want), n
        if "17x33" in n or "7x9" in n:                       # the fixture pixels stand for Pillow in the test above; here a sample decodes again
            assert np.array_equal(P.decode(d), want), n


def test_parse_gives_the_scans_of_simple_progression(cases):
    rst = {}
    for n, meta in zip(_names(cases), cases["meta"].tolist()):
        h, w, nc, hs, vs, ri, nq, ns, _ = meta
        d = cases["file_" + n].tobytes()
        info = J.parse(d, progressive=True)
        assert J.supported(d, progressive=True)
        assert (info.height, info.width, len(info.components), info.precision) == (h, w, nc, 8), n
        assert (info.components[0].h, info.components[0].v) == (hs, vs), n
        assert len(info.qtables) == nq and len(info.scans) == ns, n
        assert [(s.components, s.ss, s.se, s.ah, s.al) for s in info.scans] == (YCC_SCRIPT if nc == 3 else GRAY_SCRIPT), n
        if "rstrow" not in n:                                # restart_marker_rows: libjpeg sets the interval per scan (jcmaster.c per_scan_setup), below
            assert all(s.restart_interval == ri for s in info.scans), n
        assert info.scan == (info.scans[0].range[0], info.scans[-1].range[1]) and d[info.scan[1]:] == b"\xff\xd9", n
        for a, b in zip(info.scans, info.scans[1:]):
            assert a.range[0] <= a.range[1] < b.range[0], n
        markers = []
        for s in info.scans:
            a = np.frombuffer(d[s.range[0]:s.range[1]], np.uint8)
            markers.append(int(((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)).sum()) if a.size > 1 else 0)
            gw, gh = J.scan_geometry(info, s)
            if "rstrow" in n:
                assert s.restart_interval == gw and markers[-1] == gh - 1, n
            else:
                assert markers[-1] == (-(-gw * gh // ri) - 1 if ri else 0), n
        rst[n] = markers
    # 17 x 33 at 4:2:0: the interleaved DC scans run over the 2 x 3 MCUs of the frame, the Y scans over the 3 x 5 blocks of Y's own 17 x 33
    # samples (not the 4 x 6 blocks of the padded grid), the chroma scans over 2 x 3 blocks; the interval of 2 counts each scan's own MCUs
    assert rst["grad_q75_rst2_17x33_s2"] == [2, 7, 2, 2, 7, 7, 2, 2, 2, 7]
    # one MCU row of 48 x 64 at 4:2:0: 4 MCUs in the interleaved scans, 8 blocks in the Y scans, 4 in the chroma scans (DRI changes between scans)
    info = J.parse(cases["file_grad_q75_rstrow_48x64_s2"].tobytes(), progressive=True)
    assert [s.restart_interval for s in info.scans] == [4, 8, 4, 4, 8, 8, 4, 4, 4, 8] and rst["grad_q75_rstrow_48x64_s2"] == [2, 5, 2, 2, 5, 5, 2, 2, 2, 5]
    info = J.parse(cases["file_grad_q75_17x33_s2"].tobytes(), progressive=True)
    assert [J.scan_geometry(info, s) for s in info.scans[:3]] == [(3, 2), (5, 3), (3, 2)]


def test_huffman_tables_are_recorded_per_scan(cases):
    info = J.parse(cases["file_noise_q100_17x33_s2"].tobytes(), progressive=True)
    ac = [s for s in info.scans if s.ss > 0]
    assert all(s.ta == (0,) if s.components == (0,) else s.ta == (1,) for s in ac)
    y = [s.huffman[(1, 0)] for s in ac if s.components == (0,)]               # Pillow rewrites AC slot 0 in front of every Y scan
    assert len(y) == 4
    assert any(not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])) for a, b in zip(y, y[1:]))
    assert (0, 0) in info.scans[0].huffman and (1, 0) not in info.scans[0].huffman     # only what was in force at that SOS


def test_without_the_flag_nothing_changes(cases, golden):
    d = cases["file_grad_q75_17x33_s2"].tobytes()
    with pytest.raises(J.JpegUnsupported, match=r"progressive DCT \(SOF2\) is not supported \(baseline SOF0 only\)"):
        J.parse(d)
    assert not J.supported(d) and J.supported(d, progressive=True)
    base = golden("jpeg_cases")["file_grad_q75_17x33_s2"].tobytes()
    a, b = J.parse(base), J.parse(base, progressive=True)
    assert a.scans is None and b.scans is None and a[:4] == b[:4] and a.scan == b.scan


def test_unsupported_progressions_are_named(cases):
    d = cases["file_grad_q75_17x33_s2"].tobytes()
    sos = _sos(d)
    assert all(d[p:p + 2] == b"\xff\xda" for p in sos)

    def raises(x, word):
        with pytest.raises(J.JpegUnsupported, match=word):
            J.parse(x, progressive=True)
        assert not J.supported(x, progressive=True)

    # scan 1 is Y 1-5 Ah 0 Al 2: Ss at +7, Se at +8, Ah/Al at +9 of a one-component SOS; scan 0 has three components: Ah/Al at +13
    raises(_edit(d, sos[0] + 13, 14), "scan 0 .*Al above 13")
    raises(_edit(d, sos[5] + 9, 0x20), "scan 5 .*Al = Ah - 1")
    raises(_edit(d, sos[0] + 12, 5), "scan 0 .*Ss 0 needs Se 0")
    two = d[:sos[1] + 2] + bytes([0, 10, 2, 1, 0x00, 2, 0x11]) + d[sos[1] + 7:]          # Y 1-5 with a second component put in
    raises(two, "scan 1 .*AC scan takes one component")
    raises(d[:sos[9]] + b"\xff\xd9", "incomplete progression.*coefficient 1 of component 0 stands at bit 1")
    rng = [sc.range for sc in J.parse(d, progressive=True).scans]
    raises(d[:rng[0][1]] + d[rng[1][1]:], "scan 4 .*bogus progression.*coefficient 1 .*never sent")   # Y 1-5 dropped with its DHT: the Y refinement of 1-63 stumbles
    raises(_edit(d, sos[1] + 9, 1), "scan 5 .*bogus progression.*coefficient 1 stands at bit 1")                           # Y 1-5 sent at Al 1, Y 6-63 at Al 2: the refinement of 1-63 at Ah 2 stumbles
    dqt = d.index(b"\xff\xdb")
    L = (d[dqt + 2] << 8) | d[dqt + 3]
    raises(d[:dqt] + d[dqt + 2 + L:sos[1]] + d[dqt:dqt + 2 + L] + d[sos[1]:], "DQT segment after the first SOS")
    sof = d.index(b"\xff\xc2")
    raises(_edit(d, sof + 4, 12), "12-bit")
    raises(_edit(d, sof + 1, 0xCA), r"arithmetic coding \(SOF10, progressive\)")
    raises(_edit(d, sof + 11, 0x12), "sampling")
    raises(_edit(d, sof + 9, 4), "4 components")
    dc_y = d[:sos[0] + 2] + bytes([0, 10, 2, 1, 0x00, 2, 0x10, 0, 0, 1]) + d[sos[0] + 14:]  # the first DC scan over Y and Cb only
    raises(dc_y, "scan 0 .*DC scan of some of the components")


def test_malformed_files_raise_maferror(cases):
    d = cases["file_grad_q75_17x33_s2"].tobytes()
    info = J.parse(d, progressive=True)

    def raises(x, word):
        with pytest.raises(MafError, match=word) as e:
            J.parse(x, progressive=True)
        assert not isinstance(e.value, J.JpegUnsupported)
        assert not J.supported(x, progressive=True)

    raises(d[:-2], "EOI")
    for s in info.scans:
        raises(d[:(s.range[0] + s.range[1]) // 2], "EOI|past the end")           # the file ends inside a scan
        raises(d[:s.range[0] - 5], "past the end")                               # ... and inside an SOS segment
    dht = d.index(b"\xff\xc4")
    raises(d[:dht + 10], "past the end|cut short")
    L = (d[dht + 2] << 8) | d[dht + 3]
    raises(d[:dht] + d[dht + 2 + L:], "Huffman table DC . of scan 0 is missing")


def test_a_short_last_scan_passes_the_parser(cases):
    """The gray file has 6 scans: cut in the middle of the 6th with EOI appended, every scan is still there, so the parser lets it through and
    the decoder reports the short scan.  The same cut in a 10-scan colour file removes scans 7 to 10: that is an incomplete progression, the
    parser's finding."""
    g = cases["file_gray_q75_17x33"].tobytes()
    last = J.parse(g, progressive=True).scans[5].range
    cut = g[:(last[0] + last[1]) // 2] + b"\xff\xd9"
    assert J.supported(cut, progressive=True)
    coefs, status = P.coefficients(cut)
    assert status & J.STATUS_SHORT_SCAN
    c = cases["file_grad_q75_17x33_s2"].tobytes()
    r = J.parse(c, progressive=True).scans[5].range
    with pytest.raises(J.JpegUnsupported, match="incomplete progression"):
        J.parse(c[:(r[0] + r[1]) // 2] + b"\xff\xd9", progressive=True)
    # the 6th scan of the colour file loses its second half while scans 7 to 10 stay: complete, and short in the middle
    mid = c[:(r[0] + r[1]) // 2] + c[r[1]:]
    assert J.supported(mid, progressive=True)
    assert P.coefficients(mid)[1] & J.STATUS_SHORT_SCAN


def test_blob_has_one_round_per_scan(cases, golden):
    """build_blob: scan k of every file is round k; a baseline file in the same call keeps its lanes in the baseline lane table."""
    z = cases
    base = golden("jpeg_cases")
    names = ["grad_q75_rst2_17x33_s2", "gray_q75_17x33", "noise_q100_8x8_s0"]
    datas = [z["file_" + n].tobytes() for n in names] + [base["file_grad_q75_rst2_17x33_s0"].tobytes()]
    infos = [J.parse(d, progressive=True) for d in datas]
    hdr, images, lanes, huff, quant, scan_at, prog = J.build_blob(datas, infos)
    scans, slanes, rounds = prog
    assert int(hdr["n_rounds"]) == 10 and len(rounds) == 11 and int(hdr["n_scans"]) == 26 == len(scans)
    assert (lanes["image"][lanes["image"] >= 0] == 3).all() and int((lanes["image"] == 3).sum()) == 8       # 15 MCUs, interval 2
    per_round = [int((slanes["image"][rounds[k]:rounds[k + 1]] >= 0).sum()) for k in range(10)]
    # the 4:2:0 restart file: 3, 8, 3, 3, 8, 8, 3, 3, 3, 8 lanes; the gray file one per scan for 6 scans, the 8 x 8 file one for 10
    assert per_round == [5, 10, 5, 5, 10, 10, 4, 4, 4, 9]
    for k in range(10):
        rows = slanes[rounds[k]:rounds[k + 1]]
        assert (scans["round"][rows["image"][rows["image"] >= 0]] == k).all()
    old = J.build_blob(datas[3:], infos[3:])
    assert old[6] is None and int(old[0]["n_scans"]) == 0 and int(old[0]["scans_off"]) == 0
    buf = np.zeros(int(hdr["total_bytes"]), np.uint8)
    J.fill_blob(buf, hdr, images, lanes, huff, quant, datas, infos, scan_at, prog)
    back = buf[int(hdr["scans_off"]):int(hdr["scans_off"]) + scans.nbytes].view(J.SCAN_DT)
    assert np.array_equal(back, scans)
