"""JPEG_PROGRESSIVE_FULL without a GPU: the host scan decoder, the option bit and its geometry, the coefficient-tile kernel's
per-lane logic on the CPU emulator, the class over the CPU stand-in device, and the error paths.

Every comparison is bit-exact.  Inputs and the chain that makes the expected pixels -- tests/prog_jpeg (pure Python) ->
coef_jpeg.write_jpeg (baseline, same DQT) -> the oracle -- are in tests/prog_cases.py (Pillow's files: libjpeg's default script)
and tests/prog_scripts.py (files written by tests/prog_write.py under other scan scripts: every MCU layout, DC scans split and
paired, deep successive approximation, band splits, restart intervals that move, all table ids, long EOB runs)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpegdec_amd as J
from oracle.loader import RefDecoder
from tests import coef_jpeg, prog_cases as PC, prog_jpeg, prog_scripts as PS
from tests.cases import jpeg_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = J.PROGRESSIVE_FULL
NAMES = sorted(PC.CASES)
WRITTEN = PS.NAMES + PS.LONG_NAMES                        # the files of tests/prog_scripts.py


@pytest.fixture(scope="module")
def coefsim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_coefsim.so"))
    lib.coefsim_decode.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def class_cpu():
    subprocess.run(["make", "classcpu"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return RefDecoder(False, path=os.path.join(ROOT, "tests", "class_cpu", "libjpegdec_class_cpu.so"))


def _info(jpeg):
    info = J.binding.ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    return info


def _own_extent(dec, c):
    """(block rows, block columns) of component c's own extent: ceil(w_c / 8) x ceil(h_c / 8)"""
    hs, vs = coef_jpeg.LUMA_HV[dec["sampling"]]
    ch, cv = (hs, vs) if c == 0 else (1, 1)
    wc, hc = -(-dec["width"] * ch // hs), -(-dec["height"] * cv // vs)
    return -(-hc // 8), -(-wc // 8)


# ---- the host decoder ------------------------------------------------------------------------------------------------
def _prescaled_quant(baseline):
    """the four prescaled quantisers of a baseline file, as the baseline path builds them (JDA_TB_QUANT of the table blob)"""
    p = J.PreparedImage(baseline)
    try:
        return np.frombuffer(bytes(p.tables()[10240:10752]), dtype=np.int16).reshape(4, 64).copy()
    finally:
        p.close()


@pytest.mark.parametrize("name", NAMES + WRITTEN)
def test_host_decoder_equals_the_independent_decoder(name, product_lib):
    jpeg, twin = PS.files(name)
    dec = PS.decoded(name)
    if name in PC.CASES:
        assert dec["n_scans"] == (6 if dec["sampling"] == "gray" else 10)    # libjpeg's default script
    else:
        assert dec["n_scans"] == len(PS.case(name)["script"])
    img = J.CoefImage(jpeg)
    if name not in PC.CASES:
        # the quantisers: those in force at each component's first scan -- what the writer put there (a DQT in front of a later scan, a
        # redefinition behind the first scan), found so by the independent decoder, prescaled as the baseline path prescales the twin's
        cs = PS.case(name)["set"]
        raw = prog_jpeg.decode_coefs(jpeg)
        assert raw["quant_latched"] == [[int(x) for x in cs["quant"][t]] for t in cs["quant_ids"]]
        q, ids = img.quant()
        tq = _prescaled_quant(twin)
        assert ids[:len(cs["quant_ids"])] == [0, 1, 2][:len(cs["quant_ids"])]
        for c, t in enumerate(cs["quant_ids"]):
            assert np.array_equal(q[c], tq[t]), (name, c)
    got = img.coefficients()
    want = prog_jpeg.to_library_order(dec)
    assert got.shape == want.shape == (img.info.mcus_x * img.info.mcus_y * img.info.blocks_per_mcu, 64)
    assert np.array_equal(got, want), int(np.count_nonzero((got != want).any(axis=1)))
    img.close()


@pytest.mark.parametrize("name", NAMES + WRITTEN)
def test_independent_decoder_equals_the_baseline_twin(name):
    """Pillow decodes both files to identical pixels (same coefficients); inside every component's own extent the coefficients
    agree -- the padding blocks differ legitimately: the progressive file never codes their AC terms.  For a written file the twin is
    coef_jpeg.write_jpeg of the coefficients the script sends: Pillow (libjpeg) is the third party that reads the writer's Annex G."""
    from PIL import Image
    import io
    pj, tw = PS.files(name)
    assert tw is not None
    if name not in PS.PILLOW_EXEMPT:
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(pj))), np.asarray(Image.open(io.BytesIO(tw))))
    dec, base = PS.decoded(name), coef_jpeg.decode_coefs(tw)
    assert dec["quant"] == base["quant"] and dec["quant_ids"] == base["quant_ids"]
    for c, (a, b) in enumerate(zip(dec["coefs"], base["coefs"])):
        r, w = _own_extent(dec, c)
        assert np.array_equal(a[:r, :w], b[:r, :w]), (name, c)


@pytest.mark.parametrize("name", ["gray_200x136_q85", "c444_200x136_q98_rst", "c422_200x136_q50_rst", "c420_200x136_q50_rst", "c420_17x9_q85_rst",
                                  "fx_c420__deep_sa", "fx_c440__split_dc"])
def test_files_cut_after_each_complete_scan(name, product_lib):
    """a file that ends behind a complete scan is valid and decodes to what its scans carry"""
    jpeg = PS.files(name)[0]
    dec = PS.decoded(name)
    for k in range(dec["n_scans"]):
        cut = PC.cut_after_scan(jpeg, dec, k)
        want = prog_jpeg.to_library_order(prog_jpeg.decode_coefs(cut))
        img = J.CoefImage(cut)
        assert np.array_equal(img.coefficients(), want), (name, k)
        img.close()


def test_from_coefficients_round_trip(product_lib):
    jpeg = jpeg_for("c420_333x217")
    base = coef_jpeg.decode_coefs(jpeg)
    coefs = prog_jpeg.to_library_order(base)
    img = J.CoefImage(jpeg, coefs)
    assert np.array_equal(img.coefficients(), coefs)
    q, ids = img.quant()
    p = J.PreparedImage(jpeg)
    assert np.array_equal(q.reshape(-1), np.frombuffer(bytes(p.tables()[10240:10752]), dtype=np.int16))      # JDA_TB_QUANT of the table blob
    assert ids[:3] == [0, 1, 1]
    p.close(); img.close()
    with pytest.raises(J.JdaError) as e:
        J.CoefImage(jpeg, coefs[:-1])
    assert e.value.code == 1


# ---- the option bit and the geometry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_effective_options_and_geometry(name, product_lib, oracle):
    lib = product_lib
    pj, tw = PC.files(name)
    ip, ib = _info(pj), _info(tw)
    assert ip.jpeg_type == 1 and ib.jpeg_type == 0
    assert lib.jda_effective_options(C.byref(ip), 0) == 8                    # the default: a 1/8 thumbnail of the first scan
    assert lib.jda_effective_options(C.byref(ip), FULL) == FULL
    assert lib.jda_effective_options(C.byref(ip), FULL | 64) == FULL | 64
    assert lib.jda_effective_options(C.byref(ib), FULL) == 0                 # a baseline file: the bit is cleared
    assert lib.jda_effective_options(C.byref(ib), FULL | 2) == 2
    assert lib.jda_progressive_full_requested(C.byref(ip), FULL) == 1 and lib.jda_progressive_full_requested(C.byref(ib), FULL) == 0
    assert lib.jda_progressive_full_requested(C.byref(ip), 0) == 0
    for pt in (J.RGB565_LE, J.RGB8888, J.GRAY8):
        for opt in (0, 64):
            assert J.output_geometry(ip, pt, opt | FULL) == J.output_geometry(ib, pt, opt), (pt, opt)
            assert J.output_geometry(ib, pt, opt | FULL) == J.output_geometry(ib, pt, opt)
            for max_mcus, dma in ((0, False), (3, False), (0, True)):
                a = J.draw_plan(ip, pt, opt | FULL, max_mcus, dma)
                assert np.array_equal(a, J.draw_plan(ib, pt, opt, max_mcus, dma)), (pt, opt, max_mcus, dma)
        for scale in (2, 4, 8, 2 | 8):
            with pytest.raises(J.JdaError) as e:
                J.output_geometry(ip, pt, scale | FULL)
            assert e.value.code == 3
    # .. and the reference's strip plan for that geometry (the oracle's, of the re-encoded baseline)
    base, events = PC.reencoded(name)
    assert np.array_equal(J.draw_plan(ip, J.RGB565_LE, FULL), oracle.draw_plan(base, J.RGB565_LE, 0))


# ---- the kernel's logic on the CPU -------------------------------------------------------------------------------------
def _sim(coefsim, jpeg, coefs, pt, opt, mode, shape, flags=None):
    pitch = (shape[1] + 15) & ~15
    buf = np.zeros((shape[0], pitch), np.uint8)
    rc = coefsim.coefsim_decode(jpeg, len(jpeg), coefs.ctypes.data, len(coefs), pt, opt, mode, buf.ctypes.data, pitch, 1 << 20, shape[0],
                                None if flags is None else flags.ctypes.data)
    return rc, buf[:, :shape[1]]


@pytest.mark.parametrize("name", NAMES + WRITTEN)
def test_lane_schedule_equals_the_oracle_and_the_twin(name, product_lib, coefsim, oracle):
    """the coefficients come from the product's own scan decoder here (J.CoefImage), so that a scan decoder that differs from the independent
    one shows in the pixels too"""
    pj = PS.files(name)[0]
    base, events = PS.reencoded(name)
    assert events == 0, "the re-encoded baseline has %d truncation events: its pixels are not the coefficients' (SURVEY fact 6)" % events
    coefs = prog_jpeg.to_library_order(PS.decoded(name))
    n, ocoefs, oflags, _, _ = oracle.entropy(base)
    assert n == len(coefs) and np.array_equal(ocoefs, coefs)                  # the re-encoded baseline carries exactly these coefficients
    if name not in PC.CASES:
        img = J.CoefImage(pj)
        coefs = img.coefficients().copy()
        img.close()
        # (the emulator takes geometry and quantisers from a file's header by the baseline path's rules, which a written file's tables need not
        # meet: it gets the re-encoded baseline, whose quantisers are the latched ones -- test_host_decoder_equals_the_independent_decoder)
        pj = base
    modes = ((J.RGB8888, 0), (J.RGB565_LE, 0), (J.RGB565_BE, 0), (J.GRAY8, 0), (J.RGB565_LE, J.LUMA_ONLY))
    for pt, opt in modes[:1] if name in PS.LONG_NAMES else modes:
        orc, want, err = oracle.decode_canvas(base, pt, opt)
        assert orc == 1
        flags = np.zeros(len(coefs), np.uint32)
        rc, lanes = _sim(coefsim, pj, coefs, pt, opt | FULL, 0, want.shape, flags)
        assert rc == 0 and np.array_equal(lanes, want), (name, pt, opt, rc)
        rc, twin = _sim(coefsim, pj, coefs, pt, opt | FULL, 1, want.shape)
        assert rc == 0 and np.array_equal(twin, lanes), (name, pt, opt, rc)
        if pt == J.RGB8888:
            # the load phase's flags are the ones JPEGDecodeMCU forms for the re-encoded baseline (the oracle's restatement)
            assert np.array_equal(flags.astype(np.uint16), oflags) and int(flags.max()) <= 0xFFFF


@pytest.mark.parametrize("name", PC.BASELINE_FIXTURES + PC.STRESS_FIXTURES)
def test_lane_schedule_on_baseline_coefficients(name, product_lib, coefsim, oracle):
    """jda_coef_image_from_coefficients over existing baseline fixtures: all five layouts, 8- and 16-bit quantisers, stress streams"""
    jpeg, coefs = PC.fixture_coefs(name, oracle)
    for pt in (J.RGB8888, J.RGB565_LE, J.GRAY8):
        orc, want, err = oracle.decode_canvas(jpeg, pt, 0)
        assert orc == 1
        for mode in (0, 1):
            rc, got = _sim(coefsim, jpeg, coefs, pt, 0, mode, want.shape)
            assert rc == 0 and np.array_equal(got, want), (name, pt, mode, rc)


def test_sim_refuses_scaled_output(product_lib, coefsim):
    pj = PC.files("c420_17x9_q85_rst")[0]
    coefs = prog_jpeg.to_library_order(PC.decoded("c420_17x9_q85_rst"))
    assert _sim(coefsim, pj, coefs, J.RGB8888, J.SCALE_HALF | FULL, 0, (16, 128))[0] == 3


# ---- the class over the CPU stand-in device ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gray_200x136_q85", "c444_333x217_q85", "c422_200x136_q50_rst", "c420_640x368_q85", "c420_17x9_q85_rst"] + PS.ONE_PER_LAYOUT)
def test_class_cpu_build_walks(name, class_cpu, oracle):
    pj = PS.files(name)[0]
    base, events = PS.reencoded(name)
    assert events == 0
    gray = PS.decoded(name)["sampling"] == "gray"
    for pt, opt, max_mcus in ((J.RGB565_LE, 0, 0), (J.RGB8888, 0, 3), (J.GRAY8, 0, 0), (J.RGB565_BE, 128, 0), (J.RGB565_LE, 64, 0)):
        if gray and pt == J.RGB8888:
            continue
        orc, want, err = oracle.decode_canvas(base, pt, opt & 64)
        g = J.output_geometry(_info(base), pt, opt & 64)
        assert orc == 1 and want.shape == (g["canvas_h"], g["canvas_w"] * g["bpp"])
        shape = (g["canvas_h"], g["canvas_w"] + 64)          # (strips may overhang the padded width when the MCU count per strip does not divide it)
        a = class_cpu.decode_cb(pj, pt, opt | FULL, max_mcus=max_mcus, want_log=True, canvas_shape=shape)
        b = class_cpu.decode_cb(base, pt, opt, max_mcus=max_mcus, want_log=True, canvas_shape=shape)
        assert a["rc"] == 1 and b["rc"] == 1, (a["rc"], a["last_error"], b["rc"])
        assert np.array_equal(a["log"], b["log"]) and a["n_calls"] == b["n_calls"] and a["dma_reuse"] == b["dma_reuse"]
        if max_mcus == 0 and not (opt & 128):
            assert np.array_equal(a["log"], oracle.draw_plan(base, pt, opt & 64))
        vis = g["out_h"]                                     # (a strip's iHeight is trimmed to the visible rows, jpeg.inl:5318-5320)
        assert np.array_equal(a["canvas"][:vis, :want.shape[1]], want[:vis]), (name, pt, opt)
        assert np.array_equal(a["canvas"], b["canvas"])
        # framebuffer mode: the layout of a baseline file of that geometry
        rc1, fb1 = class_cpu.decode_fb(pj, pt, opt | FULL, fill=0x5A)
        rc2, fb2 = class_cpu.decode_fb(base, pt, opt, fill=0x5A)
        assert rc1 == 1 and rc2 == 1 and np.array_equal(fb1, fb2), (name, pt, opt, rc1, rc2)
        # without the bit: still the 1/8 thumbnail of the first scan
        if gray or (pt != J.GRAY8 and not opt & 64):      # (a colour progressive file to 8-bit gray: refused)
            t = class_cpu.decode_cb(pj, pt, opt, want_log=True)
            orc, thumb, err = oracle.decode_canvas(pj, pt, opt & 64)
            assert t["rc"] == 1 and t["scale_shift"] == 3 and orc == 1
            assert np.array_equal(t["canvas"][:(g["out_h"] + 7) // 8, :thumb.shape[1]], thumb[:(g["out_h"] + 7) // 8])


def test_class_cpu_build_refusals(class_cpu):
    from tests.orient_util import with_orientation
    pj = PC.files("c420_200x136_q50_rst")[0]
    r = class_cpu.decode_cb(pj, J.RGB565_LE, FULL, crop=(16, 16, 64, 64), canvas_shape=(400, 2600))
    assert r["rc"] == 0 and r["last_error"] == 3
    for scale in (2, 4, 8):
        r = class_cpu.decode_cb(pj, J.RGB565_LE, FULL | scale, canvas_shape=(400, 2600))
        assert r["rc"] == 0 and r["last_error"] == 3, scale
    r = class_cpu.decode_cb(pj, J.RGB565_LE, FULL | 32, canvas_shape=(400, 2600))                # JPEG_EXIF_THUMBNAIL
    assert r["rc"] == 0 and r["last_error"] == 3
    turned = with_orientation(pj, 6)
    r = class_cpu.decode_cb(turned, J.RGB565_LE, FULL | 1, canvas_shape=(400, 2600))           # JPEG_AUTO_ROTATE on an orientation 2..8
    assert r["rc"] == 0 and r["last_error"] == 3
    r = class_cpu.decode_cb(with_orientation(pj, 1), J.RGB565_LE, FULL | 1, canvas_shape=(400, 2600))
    assert r["rc"] == 1                                                                       # (an orientation that changes nothing)
    # a scan that cannot be decoded: nothing is delivered, the framebuffer is untouched
    bad = _broken(pj)
    r = class_cpu.decode_cb(bad, J.RGB565_LE, FULL, want_log=True, canvas_shape=(400, 2600))
    assert r["rc"] == 0 and r["last_error"] == 2 and r["n_calls"] == 0
    rc, fb = class_cpu.decode_fb(bad, J.RGB565_LE, FULL, fill=0x5A)
    assert rc == 0 and class_cpu.last_error == 2 and bool((fb == 0x5A).all())


# ---- error paths ------------------------------------------------------------------------------------------------------
def _broken(jpeg):
    """the file with one bit of its first scan flipped so that the scan runs into an invalid Huffman code (the independent decoder says so)"""
    dec = prog_jpeg.decode_coefs(jpeg)
    b = bytearray(jpeg)
    for at in range(dec["scan_ends"][0] - 1, 0, -1):       # a byte of the first scan whose flip the independent decoder refuses
        if b[at] in (0xFF, 0x00) or b[at - 1] == 0xFF:
            continue
        for bit in (0x80, 0x40, 0x20, 0x10):
            c = bytearray(b)
            c[at] ^= bit
            if c[at] == 0xFF:
                continue
            try:
                prog_jpeg.decode_coefs(bytes(c))
            except coef_jpeg.DecodeError:
                return bytes(c)
    raise AssertionError("no flip of the first scan breaks it")


def test_error_paths(product_lib):
    pj, tw = PC.files("c444_333x217_q85")
    with pytest.raises(J.JdaError) as e:
        J.CoefImage(tw)                                    # a baseline file
    assert e.value.code == 1
    with pytest.raises(J.JdaError) as e:
        J.CoefImage(_broken(pj))                           # a flipped Huffman byte
    assert e.value.code == 2
    # scan headers against the band rules (a DC band that ends at 5 in the first scan; an AC band of the second scan that ends in front
    # of its start), and one naming a component the frame does not have
    at = pj.index(b"\xff\xda")
    ns = pj[at + 4]
    at2 = prog_jpeg.decode_coefs(pj)["scan_ends"][0]
    while pj[at2:at2 + 2] != b"\xff\xda":                  # (a DHT segment stands between the scans)
        at2 += 2 + ((pj[at2 + 2] << 8) | pj[at2 + 3])
    ns2 = pj[at2 + 4]
    assert pj[at2 + 5 + 2 * ns2] > 0                       # Ss of an AC scan
    for off, val in ((at + 5 + 2 * ns + 1, 5), (at + 5, 0x77), (at2 + 5 + 2 * ns2 + 1, 0), (at2 + 5, 0x77)):
        b = bytearray(pj)
        b[off] = val
        with pytest.raises(J.JdaError) as e:
            J.CoefImage(bytes(b))
        assert e.value.code == 2, off


# ---- tables between the scans ------------------------------------------------------------------------------------------
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def remap_table_ids(jpeg):
    """the file with the chroma DC table of its first scan moved to id 3 and the AC table of its second scan to id 2 (the DHT segments and
    the scan headers rewritten): ids the baseline path's LUT storage does not have"""
    b = bytearray(jpeg)
    segs = prog_jpeg._segments(jpeg)
    sos = [k for k, sg in enumerate(segs) if sg[0] == 0xDA]
    moved = 0
    for m, off, ln, ent in segs[:sos[0]]:                  # the DC table 1 in front of the first scan (Pillow writes one table a segment)
        if m == 0xC4 and b[off] == 0x01:
            b[off] = 0x03
            moved += 1
    m, off, ln, ent = segs[sos[0]]
    for k in range(b[off]):
        if b[off + 2 + 2 * k] >> 4 == 1:
            b[off + 2 + 2 * k] = (3 << 4) | (b[off + 2 + 2 * k] & 15)
            moved += 1
    for m, off, ln, ent in segs[sos[0] + 1:sos[1]]:        # the AC table in front of the second scan
        if m == 0xC4 and b[off] >> 4 == 1:
            old = b[off] & 15
            b[off] = 0x12
            m2, off2, ln2, ent2 = segs[sos[1]]
            assert b[off2] == 1 and b[off2 + 2] & 15 == old
            b[off2 + 2] = (b[off2 + 2] & 0xF0) | 2
            moved += 1
    assert moved >= 3
    return bytes(b)


def with_dqt_behind_first_scan(jpeg, table, values):
    """the file with a DQT segment (8-bit, `values` in zigzag order) inserted right behind its first scan"""
    at = prog_jpeg.decode_coefs(jpeg)["scan_ends"][0]
    return jpeg[:at] + _seg(0xDB, bytes([table]) + bytes(values)) + jpeg[at:]


def without_header_dqt(jpeg, table):
    """the file without the header's DQT of `table` (Pillow writes one table a segment)"""
    for m, off, ln, ent in prog_jpeg._segments(jpeg):
        if m == 0xDB and jpeg[off] == table and ln == 65:
            return jpeg[:off - 4] + jpeg[off + ln:]
    raise AssertionError("no such DQT")


@pytest.mark.parametrize("name", ["c420_200x136_q50_rst", "c444_333x217_q85"])
def test_huffman_table_ids_2_and_3(name, product_lib, coefsim, oracle):
    pj = PC.files(name)[0]
    moved = remap_table_ids(pj)
    assert moved != pj
    a, b = J.CoefImage(pj), J.CoefImage(moved)
    assert np.array_equal(a.coefficients(), b.coefficients()) and np.array_equal(a.quant()[0], b.quant()[0])
    assert np.array_equal(prog_jpeg.to_library_order(prog_jpeg.decode_coefs(moved)), b.coefficients())
    a.close(); b.close()
    # .. also with unused tables of ids 2 and 3 in the header
    seg = prog_jpeg._segments(pj)
    first_dht = [sg for sg in seg if sg[0] == 0xC4][0]
    body = pj[first_dht[1] + 1:first_dht[1] + first_dht[2]]
    extra = pj[:first_dht[1] - 4] + _seg(0xC4, bytes([0x02]) + body) + _seg(0xC4, bytes([0x03]) + body) + pj[first_dht[1] - 4:]
    c = J.CoefImage(extra)
    assert np.array_equal(c.coefficients(), prog_jpeg.to_library_order(PC.decoded(name)))
    c.close()


def test_quantisers_are_latched_at_a_components_first_scan(product_lib, coefsim, oracle):
    name = "c420_200x136_q50_rst"
    pj = PC.files(name)[0]
    dec = PC.decoded(name)
    base, events = PC.reencoded(name)
    assert events == 0
    ref = J.CoefImage(pj)
    q_ref, ids = ref.quant()
    assert ids == [0, 1, 2]                                # table c of the image = component c's
    # the header's quantisers, prescaled as the baseline path prescales them (the twin's table blob)
    twin = J.PreparedImage(PC.files(name)[1])
    tq = np.frombuffer(bytes(twin.tables()[10240:10752]), dtype=np.int16).reshape(4, 64)
    assert np.array_equal(q_ref[0], tq[0]) and np.array_equal(q_ref[1], tq[1]) and np.array_equal(q_ref[2], tq[1])
    twin.close()
    # a DQT behind the first scan redefines a table: every component was named by the first scan, its quantiser stays what it was
    for table in (0, 1):
        late = with_dqt_behind_first_scan(pj, table, [255] * 64)
        img = J.CoefImage(late)
        assert np.array_equal(img.quant()[0], q_ref) and np.array_equal(img.coefficients(), ref.coefficients()), table
        orc, want, err = oracle.decode_canvas(base, J.RGB8888, 0)
        rc, got = _sim(coefsim, late, img.coefficients(), J.RGB8888, FULL, 0, want.shape)
        img.close()
    # the chroma table defined only behind the first scan, which names the chroma components: no quantiser in force, JDA_DECODE_ERROR
    chroma = dec["quant"][1]
    orphan = with_dqt_behind_first_scan(without_header_dqt(pj, 1), 1, chroma)
    with pytest.raises(J.JdaError) as e:
        J.CoefImage(orphan)
    assert e.value.code == 2
    # .. and defined in the header AND redefined in front of the first SOS: the later one is in force
    at = pj.index(b"\xff\xda")
    twice = without_header_dqt(pj, 1)
    at = twice.index(b"\xff\xda")
    twice = twice[:at] + _seg(0xDB, bytes([1]) + bytes([255] * 64)) + _seg(0xDB, bytes([1]) + bytes(chroma)) + twice[at:]
    img = J.CoefImage(twice)
    assert np.array_equal(img.quant()[0], q_ref)
    img.close(); ref.close()


def test_a_file_cut_inside_a_scan_is_read_with_zero_bits(product_lib):
    """documented behaviour (include/jpegdec_amd.h): the scan the data ends in is decoded as if zero bits followed, as libjpeg does"""
    name = "c420_200x136_q50_rst"
    pj, dec = PC.files(name)[0], PC.decoded(name)
    cut = pj[:(dec["scan_ends"][2] + dec["scan_ends"][3]) // 2]
    img = J.CoefImage(cut)
    assert img.coefficients().shape == (prog_jpeg.to_library_order(dec).shape)
    img.close()


# ---- the written files (tests/prog_write.py, tests/prog_scripts.py) -------------------------------------------------------------------------
@pytest.mark.parametrize("name", WRITTEN)
def test_written_files_hold_the_coefficients_their_script_sends(name):
    """the independent decoder reads back what went in, over the whole MCU grid: the input inside each component's own extent, truncated to
    the lowest bit sent; zero in the bands, components and padding blocks that no scan carries"""
    c = PS.case(name)
    dec = prog_jpeg.decode_coefs(c["jpeg"])
    cs = c["set"]
    assert (dec["width"], dec["height"], dec["sampling"]) == (cs["width"], cs["height"], cs["sampling"])
    sent = np.zeros((len(cs["coefs"]), 64), bool)
    for sc in c["script"]:
        for comp in sc["comps"]:
            sent[comp, sc["ss"]:sc["se"] + 1] = True
    final = all(sc["al"] == 0 for sc in c["script"] if not any(o["ss"] == sc["ss"] and o["comps"] == sc["comps"] and o["ah"] == sc["al"] and o["ah"] for o in c["script"]))
    for k, (got, eff, src) in enumerate(zip(dec["coefs"], c["effective"], cs["coefs"])):
        assert np.array_equal(got, eff), (name, k)
        r, w = _own_extent(dec, k)
        assert not got[..., ~sent[k]].any()
        if final:                                           # every band that was sent was sent down to bit 0
            assert np.array_equal(got[:r, :w][..., sent[k]], np.asarray(src)[:r, :w][..., sent[k]]), (name, k)


def test_pillow_exemptions_are_bounded():
    """the third-party anchor may leave out only DC-edge stress sets and the long-EOB files, by name; as it stands it leaves out none"""
    assert set(PS.PILLOW_EXEMPT) <= set(PS.PILLOW_EXEMPT_ALLOWED)
    assert all(n.startswith(("k_fastbound_dc_", "k_dcdrift_", "long_eob_")) for n in PS.PILLOW_EXEMPT_ALLOWED)
    assert len(PS.PILLOW_EXEMPT) == 0


@pytest.mark.parametrize("path", sorted(PS.PATHS))
def test_written_files_reach_the_paths_they_exist_for(path):
    """measured from the writer's own symbol log, so that a change to a generator cannot silently stop exercising the path"""
    name, measure, holds = PS.PATHS[path]
    value = measure(PS.case(name)["log"])
    assert holds(value), "%s in %s: measured %r" % (path, name, value)


def test_every_layout_has_written_files():
    layouts = {}
    for name in PS.NAMES:
        layouts.setdefault(PS.case(name)["set"]["sampling"], []).append(name)
    assert sorted(layouts) == sorted(coef_jpeg.LAYOUTS), sorted(layouts)
    n440 = len(layouts["4:4:0"])
    assert n440 >= 10, "4:4:0 files: %d" % n440
    info = _info(PS.files(PS.ONE_PER_LAYOUT[3])[0])
    assert info.subsample == 0x12 and info.jpeg_type == 1


@pytest.mark.parametrize("name", PS.NAMES)
def test_without_the_bit_the_answer_is_the_references(name, class_cpu, oracle):
    """without JPEG_PROGRESSIVE_FULL a written file gets what the reference gives it -- the 1/8 thumbnail of the first scan where that scan is
    the DC scan of every component, and the reference's return code and pixels whatever the first scan is"""
    pj = PS.files(name)[0]
    gray = PS.decoded(name)["sampling"] == "gray"
    for pt in (J.RGB565_LE, J.RGB8888) + ((J.GRAY8,) if gray else ()):
        if gray and pt == J.RGB8888:
            continue
        orc, thumb, err = oracle.decode_canvas(pj, pt, 0)
        t = class_cpu.decode_cb(pj, pt, 0, want_log=True)
        assert t["rc"] == orc, (name, pt, t["rc"], t["last_error"], orc, err)
        if PS.NEW[name][1] in PS.FIRST_SCAN_ALL_DC:
            assert orc == 1 and t["scale_shift"] == 3
        elif PS.NEW[name][1] == "tables":                  # (DC tables of ids 2 and 3 in the header: the reference has no room for them)
            assert orc == 0 and err == 3
        if orc == 1:
            g = J.output_geometry(_info(pj), pt, J.SCALE_EIGHTH)
            assert np.array_equal(t["canvas"][:g["out_h"], :thumb.shape[1]], thumb[:g["out_h"]]), (name, pt)
        else:
            assert t["last_error"] == err, (name, pt, t["last_error"], err)


@pytest.mark.parametrize("kind", sorted(PS.malformed()))
def test_malformed_scans_are_refused(kind, product_lib, class_cpu):
    """Annex G's error exits: JDA_DECODE_ERROR from the host decoder, DecodeError from the independent one; nothing reaches a kernel"""
    bad = PS.malformed()[kind]
    with pytest.raises(coef_jpeg.DecodeError):
        prog_jpeg.decode_coefs(bad)
    with pytest.raises(J.JdaError) as e:
        J.CoefImage(bad)
    assert e.value.code == 2
    r = class_cpu.decode_cb(bad, J.RGB565_LE, FULL, want_log=True, canvas_shape=(400, 2600))
    assert r["rc"] == 0 and r["last_error"] == 2 and r["n_calls"] == 0
    rc, fb = class_cpu.decode_fb(bad, J.RGB565_LE, FULL, fill=0x5A)
    assert rc == 0 and class_cpu.last_error == 2 and bool((fb == 0x5A).all())


def test_malformed_files_come_from_valid_ones(product_lib):
    """each malformed file differs from a file the decoder accepts only by the writer's malform hook: the same scripts without it decode"""
    cs = PS.coef_set("fx_c420")
    for script in (PS._deep_sa(3, cs["quant"])[0][:8], PS._seq(3, cs["quant"])[0], PS._pair(3, cs["quant"])[0], [PS.scan((0, 1, 2), 0, 0, 0, 13)]):
        ok = PS.PW.write_progressive(cs["width"], cs["height"], cs["sampling"], cs["coefs"], cs["quant"], cs["quant_ids"], script)
        img = J.CoefImage(ok)
        assert np.array_equal(img.coefficients(), prog_jpeg.to_library_order(prog_jpeg.decode_coefs(ok)))
        img.close()


def test_ac_first_pass_values_that_leave_int16_wrap(product_lib):
    """documented behaviour (include/jpegdec_amd.h): value << Al is kept modulo 2^16, at coefficient level only -- no pixels are promised"""
    jpeg, eff = PS.wrap_case()
    dec = prog_jpeg.decode_coefs(jpeg)
    assert np.array_equal(dec["coefs"][0], eff[0]) and int(eff[0].max()) == 40000 and int(eff[0].min()) == -40000
    img = J.CoefImage(jpeg)
    got, want = img.coefficients(), prog_jpeg.to_library_order(dec)
    assert np.array_equal(got, want)
    assert sorted(int(v) for v in got[got != 0] if abs(int(v)) > 20000) == [-25536, 25536, 32766]
    img.close()


def test_written_and_malformed_files_under_asan_ubsan(class_cpu, tmp_path):
    """every written file and every malformed one once through the sanitizer build of the class and the host decoder, with the bit (callbacks
    and framebuffer) and without it"""
    files = [PS.files(n)[0] for n in PS.NAMES + PS.LONG_NAMES[:1]] + [PS.malformed()[k] for k in sorted(PS.malformed())] + [PS.wrap_case()[0]]
    lines = []
    for k, f in enumerate(files):
        (tmp_path / ("img%d.jpg" % k)).write_bytes(f)
        lines += ["W %d 0 0 %d 0 0 0 -1 -1 -1 -1" % (k, FULL), "W %d 1 2 %d 0 0 0 -1 -1 -1 -1" % (k, FULL), "W %d 0 0 0 0 0 0 -1 -1 -1 -1" % k]
    (tmp_path / "walks.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "class_cpu", "walks_asan"), str(tmp_path), str(len(files))], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=1200)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "walks done" in r.stdout and int(r.stdout.split("walks done")[0].split()[-1]) == len(lines), r.stdout[-300:]
