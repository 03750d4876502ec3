"""The sparse coefficient form and the load phase of jda_sparse_tiles without a GPU: the host pack (jda_coef_image_sparse), the kernel's own
jda_cs_* functions lane by lane on the CPU (tests/hostsim/coef_sparse_sim.cpp: LDS poisoned before every tile, every global load held to
the uploaded allocation and to its alignment) against the dense load phase and the row-major twin, the choice JDA_COEF_AUTO makes, the
tile lists of a rectangle, the refusals, and the same pack and load phase as a program of its own under AddressSanitizer + UBSan.

Every comparison is bit-exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpegdec_amd as J
from tests import prog_cases as PC, prog_scripts as PS, sparse_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = PC.BASELINE_FIXTURES + PC.STRESS_FIXTURES
PILLOW = sorted(PC.CASES)
WRITTEN = PS.NAMES + PS.LONG_NAMES
MODE_OF = {0x00: "gray", 0x11: "4:4:4", 0x21: "4:2:2", 0x12: "4:4:0", 0x22: "4:2:0"}


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_coefsparsesim.so"))
    lib.coefsparsesim_run.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.coefsparsesim_plan_tiles.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def twin(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_coefsim.so"))
    lib.coefsim_decode.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def _image(kind, name, oracle):
    """(jpeg, CoefImage) of a baseline fixture (its coefficients through from_coefficients) or of a progressive file (every scan decoded)"""
    if kind == "fixture":
        jpeg, coefs = PC.fixture_coefs(name, oracle)
        return jpeg, J.CoefImage(jpeg, coefs)
    jpeg = (PC.files(name) if kind == "pillow" else PS.files(name))[0]
    return jpeg, J.CoefImage(jpeg)


ALL_IMAGES = [("fixture", n) for n in FIXTURES] + [("pillow", n) for n in PILLOW] + [("written", n) for n in WRITTEN]


def _canvas(g):
    pitch = (g["canvas_w"] * g["bpp"] + 15) & ~15
    buf = np.zeros(pitch * g["canvas_h"] + 16, np.uint8)
    off = (-buf.ctypes.data) & 15
    return buf[off:off + pitch * g["canvas_h"]].reshape(g["canvas_h"], pitch), pitch


def _run(sim, jpeg, coefs, pt, opt, geometry=None, rect=None):
    """the simulated sparse load phase (compared with the dense one inside) over every tile; with `geometry` also the pixels"""
    info = (C.c_int32 * 3)()
    coefs = None if coefs is None else np.ascontiguousarray(coefs)      # (None: every scan of the progressive file, decoded by the library)
    cp, cn = (None, 0) if coefs is None else (coefs.ctypes.data, coefs.shape[0])
    r = None if rect is None else (C.c_int32 * 4)(*rect)
    if geometry is None:
        rc = sim.coefsparsesim_run(jpeg, len(jpeg), cp, cn, pt, opt, r, None, 0, 0, 0, info)
        return rc, list(info), None
    out, pitch = _canvas(geometry)
    rc = sim.coefsparsesim_run(jpeg, len(jpeg), cp, cn, pt, opt, r, out.ctypes.data, pitch, geometry["canvas_w"], geometry["canvas_h"], info)
    return rc, list(info), out[:, :geometry["canvas_w"] * geometry["bpp"]].copy()


def _twin(twin, jpeg, coefs, pt, opt, geometry):
    out, pitch = _canvas(geometry)
    coefs = np.ascontiguousarray(coefs)
    rc = twin.coefsim_decode(jpeg, len(jpeg), coefs.ctypes.data, coefs.shape[0], pt, opt, 1, out.ctypes.data, pitch, geometry["canvas_w"], geometry["canvas_h"], None)
    assert rc == 0
    return out[:, :geometry["canvas_w"] * geometry["bpp"]].copy()


# ---- 1. the format ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", ALL_IMAGES)
def test_sparse_form(kind, name, product_lib, oracle):
    jpeg, im = _image(kind, name, oracle)
    try:
        dense = im.coefficients()
        first, entries = im.sparse()
        nb = dense.shape[0]
        assert first.shape == (nb + 1,) and first[0] == 0 and first[nb] == entries.size
        assert bool((np.diff(first.astype(np.int64)) >= 0).all())                      # monotone
        block = np.repeat(np.arange(nb, dtype=np.int64), np.diff(first.astype(np.int64)))
        assert np.array_equal(entries >> 22, (block & 1023).astype(np.uint32))         # the block bits
        n = ((entries >> 16) & 63).astype(np.int64)
        assert bool(((entries & 0xFFFF) != 0).all())                                   # no zero-valued entry
        same_block = block[1:] == block[:-1]
        assert bool((n[1:][same_block] > n[:-1][same_block]).all())                    # ascending within a block
        back = np.zeros((nb, 64), np.uint16)
        back[block, n] = (entries & 0xFFFF).astype(np.uint16)
        assert np.array_equal(back.view(np.int16), dense)
        assert entries.size == int(np.count_nonzero(dense))
        a16 = lambda v: (v + 15) & ~15
        assert im.sparse_bytes() == a16(4 * (nb + 1)) + a16(4 * entries.size)
        assert product_lib.jda_coef_image_sparse_status(im.handle) == 0
        f2, e2 = im.sparse()                                                           # cached: the same arrays
        assert f2.ctypes.data == first.ctypes.data and (e2.size == 0 or e2.ctypes.data == entries.ctypes.data)
    finally:
        im.close()


# ---- 2. the load phase = the dense load phase ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [(k, n) for k, n in ALL_IMAGES if n not in PS.LONG_NAMES])
def test_load_phase_equals_the_dense_load_phase(kind, name, sim, product_lib, oracle):
    """slots and chunk words behind jda_cs_zero + jda_cs_scatter == those behind jda_ct_load, for every tile (the fixtures and files cover
    all five layouts); no load leaves the allocation or its alignment"""
    jpeg, im = _image(kind, name, oracle)
    try:
        I = im.info
        per = SC.MCUS_PER_TILE[MODE_OF[I.subsample] if I.ncomp == 3 else "gray"]
        rc, info, _ = _run(sim, jpeg, im.coefficients() if kind == "fixture" else None, J.RGB565_LE, 0)
        assert rc == 0, (name, rc, info)
        assert info[0] == I.mcus_y * -(-I.mcus_x // per)
    finally:
        im.close()


def test_every_layout_is_among_them(product_lib, oracle):
    seen = set()
    for n in FIXTURES:
        jpeg = PC.fixture_jpeg(n)
        info = J.binding.ImageInfo()
        assert product_lib.jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
        seen.add("gray" if info.ncomp == 1 else MODE_OF[info.subsample])
    assert seen == set(SC.NBLK)


# ---- 3. the edge sets --------------------------------------------------------------------------------------------------------------------
EDGE_LABELS = [s[0] for s in SC.edge_sets()]


@pytest.mark.parametrize("label", EDGE_LABELS)
def test_edge_sets(label, sim, twin, product_lib):
    _, jpeg, coefs, pt, opt = [s for s in SC.edge_sets() if s[0] == label][0]
    im = J.CoefImage(jpeg, coefs)
    try:
        g = im.geometry(pt, opt)
        first, entries = im.sparse()
        lens = np.diff(first.astype(np.int64))
        if label.startswith("empty_"):
            assert entries.size == (1 if label == "empty_then_one" else 0)
        if label == "full_beside_empty":
            assert sorted(set(lens.tolist())) == [0, 64]
        if label == "gray_full_tile":
            assert bool((lens[:64] == 64).all()) and first[64] == 4096
        if label == "ranges":
            starts = first[::64]
            assert np.diff(starts.astype(np.int64)).tolist() == SC.RANGE_LENGTHS
            assert (starts[:-1] % 4).tolist() == SC.RANGE_STARTS_MOD4 and {1, 2, 3} <= set((starts[:-1] % 4).tolist())
        if label == "values":
            assert {0x8000, 0xFFFF, 1} <= set((entries & 0xFFFF).tolist())
        if label == "wrap_264":
            assert im.info.mcus_x == 33 and coefs.shape[0] == 1089
            e = entries[first[1023]:first[1056]]
            assert bool((np.diff((e >> 22).astype(np.int64)) < 0).any()) and (e >> 22).max() == 1023 and (e >> 22).min() == 0      # the bits wrap inside the tile
        rc, info, got = _run(sim, jpeg, coefs, pt, opt, g)
        assert rc == 0, (label, rc, info)
        if label == "gray_full_tile":
            assert info[2] == 4096
        want = _twin(twin, jpeg, coefs, pt, opt, g)
        assert np.array_equal(got, want), (label, int(np.count_nonzero(got != want)))
    finally:
        im.close()


# ---- 4. JDA_COEF_AUTO --------------------------------------------------------------------------------------------------------------------
def _auto(im):
    """(the form JDA_COEF_AUTO makes resident, its bytes behind the quantisers) by the documented rule (include/jpegdec_amd.h): fewer bytes,
    dense on a tie -- host-only byte counts; tests/test_gpu_sparse_coef.py holds jda_coef_upload_ex to the same rule on the device"""
    sp, de = im.sparse_bytes(), im.dense_bytes()
    return (J.COEF_SPARSE, sp) if sp < de else (J.COEF_DENSE, de)


def test_auto_picks_by_bytes(product_lib, oracle):
    """AUTO is the form of fewer bytes (dense on a tie).  Dense for quality-100 noise; sparse for every photograph-like file up to quality 85
    and for the photographic baseline fixtures.  (Pillow's two large quality-98 files carry sigma-3 noise at a near-lossless quality: 31-32
    nonzero terms a block, so dense is the smaller form there, by 1-2 % -- the rule, not the file's name, decides.)"""
    import io
    from PIL import Image
    rng = np.random.default_rng(7)
    b = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).save(b, "JPEG", quality=100, subsampling="4:4:4", progressive=True)
    noise = J.CoefImage(b.getvalue())
    try:
        first, entries = noise.sparse()
        assert entries.size > 31 * (first.size - 1)            # more than 31 nonzero terms a block: larger sparse than dense
        assert noise.sparse_bytes() > noise.dense_bytes() and _auto(noise) == (J.COEF_DENSE, noise.dense_bytes())
    finally:
        noise.close()
    for kind, name in [("pillow", n) for n in PILLOW] + [("fixture", n) for n in ("c444_333x217", "c420_333x217", "c420_640x368_rstrow", "gray_64x64_rst3", "c420_250x250_q10")]:
        jpeg, im = _image(kind, name, oracle)
        try:
            sp, de = im.sparse_bytes(), im.dense_bytes()
            if kind == "fixture" or PC.CASES[name][3] <= 85:
                assert sp < de and _auto(im)[0] == J.COEF_SPARSE, (name, sp, de)
        finally:
            im.close()


# ---- 5. the tile lists of a rectangle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling,mode", [("gray", 0), ("4:4:4", 1), ("4:2:0", 2), ("4:2:2", 3), ("4:4:0", 4)])
def test_rectangle_tile_lists(sampling, mode, sim):
    per = SC.MCUS_PER_TILE[sampling]
    mx, my = 2 * per + 3, 5
    first = (C.c_int32 * 2)()

    def tiles(rect):
        return sim.coefsparsesim_plan_tiles(mx, my, mode, None if rect is None else (C.c_int32 * 4)(*rect), first)

    assert tiles(None) == my * 3
    for x0, y0, x1, y1 in ((0, 0, mx, my), (1, 1, 2, 2), (3, 1, 3 + per + 1, 4), (per - 1, 0, per + 1, my), (0, 2, per, 3)):
        assert tiles((x0, y0, x1, y1)) == (y1 - y0) * -(-(x1 - x0) // per)
        assert (first[0], first[1]) == (x0, y0)                 # tiles are cut from the rectangle's own first MCU
    assert tiles((-5, -5, 10 * mx, 10 * my)) == my * 3          # clamped to the image
    assert tiles((mx - 1, my - 1, mx + 7, my + 7)) == 1
    for empty in ((3, 3, 3, 4), (4, 2, 2, 4), (0, 0, 0, 0), (mx, 0, mx + 4, my), (0, my, mx, my + 1), (-4, -4, -1, -1)):
        assert tiles(empty) == 0


def test_rectangle_through_the_load_phase(sim, twin, product_lib):
    """a rectangle changes only the tile list: the tiles inside decode to the twin's pixels, everything else keeps what was there"""
    _, jpeg, coefs, pt, opt = [s for s in SC.edge_sets() if s[0] == "rows_c420"][0]
    im = J.CoefImage(jpeg, coefs)
    try:
        g = im.geometry(pt, opt)
        want = _twin(twin, jpeg, coefs, pt, opt, g)
        rc, info, got = _run(sim, jpeg, coefs, pt, opt, g, rect=(3, 1, 11, 2))
        assert rc == 0 and info[0] == 1
        assert np.array_equal(got[16:32, 3 * 16 * 4:], want[16:32, 3 * 16 * 4:])
        got[16:32, 3 * 16 * 4:] = 0
        assert not got.any()
    finally:
        im.close()


# ---- 6. the refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(product_lib, oracle):
    lib = product_lib
    jpeg, im = _image("fixture", "c420_333x217", oracle)
    try:
        err = C.c_int32(0)
        for form in (0, 1, 2):
            assert not lib.jda_coef_upload_ex(None, im.handle, form, C.byref(err)) and err.value == 6      # JDA_ERROR_NO_DEVICE: no context
        for form in (-1, 3, 100):                              # the form and the image are checked on the host, before the context is looked at
            assert not lib.jda_coef_upload_ex(None, im.handle, form, C.byref(err)) and err.value == 1
        assert not lib.jda_coef_upload_ex(None, None, J.COEF_AUTO, C.byref(err)) and err.value == 1
        assert not lib.jda_coef_upload(None, im.handle, C.byref(err)) and err.value == 6
        assert lib.jda_coef_decode_surfaces_rect(None, 1, None, None, None, None, None) == 6
        assert lib.jda_dev_coef_form(None) == 0 and lib.jda_dev_coef_bytes(None) == 0
        assert not lib.jda_coef_image_sparse(None, None, None) and lib.jda_coef_image_sparse_bytes(None) == 0
        assert lib.jda_coef_image_sparse_status(None) == 1
    finally:
        im.close()
    with pytest.raises(ValueError):
        J.decode_to_tensors(None, [jpeg], progressive="nonsense")                     # before any GPU is touched: no context at all


def test_the_simulator_refuses_a_scale_bit_as_the_planner_does(sim, product_lib):
    """tests/hostsim/coef_sparse_sim.cpp restates the planner's rule (full size only) and is held to it here; the product's own check
    (jda_coef_plan_build, the pipeline's worker) needs resident images and is reached on the GPU: jda_coef_decode_surfaces with a scale bit in
    tests/test_gpu_progressive_full.py, status 3 of the FULL | SCALE_HALF file in tests/test_gpu_sparse_coef.py"""
    _, jpeg, coefs, pt, opt = [s for s in SC.edge_sets() if s[0] == "one_mcu_c420"][0]
    for bit in (J.SCALE_HALF, J.SCALE_QUARTER, J.SCALE_EIGHTH):
        rc, info, _ = _run(sim, jpeg, coefs, pt, bit)
        assert rc == 3


# ---- 7. pack and load phase under AddressSanitizer + UBSan: a program of its own ---------------------------------------------------------------
def test_pack_and_load_phase_under_sanitizers(tmp_path):
    subprocess.run(["make", "sparsepack"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    names = []
    for k, data in enumerate((PC.files("c420_333x217_q98")[0], PS.files("fx_c420__deep_sa")[0], PS.files(PS.LONG_NAMES[0])[0])):
        f = tmp_path / ("f%d.jpg" % k)
        f.write_bytes(data)
        names.append(str(f))
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "sparse_pack_asan")] + names, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    assert r.stdout.decode().count(": rc 0,") == 3
