"""The coefficient-level stress streams (COEF_CASES, tests/coef_jpeg.py) on the GPU: bit-exact with the oracle -- which
tests/test_coef_streams_cpu.py pins to the real reference on the same corpus -- in every pixel type and scale (the decode,
1/4-scale and DC-thumbnail kernels through their options), through the device pre-scan, the streamed pipeline and P1 in
chunks; and with oracle/_ref itself where it travelled."""
import numpy as np
import pytest

import jpegdec_amd as J
from tests.cases import COEF_CASES, COEF_CORRUPT, RUNONLY_CASES, all_modes, coef_jpeg_for, jpeg_for

pytestmark = pytest.mark.gpu

GOOD = sorted(k for k in COEF_CASES if k not in COEF_CORRUPT)


def _leaves_int16(name):
    if not name.startswith("k_dcdrift_"):
        return False
    target = int(name.split("_")[3])
    return target > 32767 or target < -32768


@pytest.mark.parametrize("name", sorted(COEF_CASES))
def test_decode_to_host_all_modes(name, gpu_ctx, oracle):
    jpeg = coef_jpeg_for(name)
    for pt, opt in all_modes(name):
        orc, want, err = oracle.decode_canvas(jpeg, pt, opt)
        rc, got, g = J.decode_to_host(gpu_ctx, jpeg, pt, opt)
        assert (rc == 0) == (orc == 1), (name, pt, opt, rc, orc, err)
        if name not in COEF_CORRUPT:
            assert orc == 1, (name, pt, opt, err)
        if orc == 1:
            assert got.shape == want.shape
            assert np.array_equal(got, want), "%s pt=%d opt=%d: %d differing bytes" % (name, pt, opt, int(np.count_nonzero(got != want)))


def test_decode_matches_real_reference_when_present(gpu_ctx, ref_scalar):
    """the families against oracle/_ref itself, one case of each per layout"""
    names = [k for k in GOOD if k.startswith(("k_classes_", "k_single_q255_", "k_fastbound_ac_", "k_huff_custom_", "k_edge_"))]
    names += [k for k in GOOD if k.startswith("k_dcdrift_c420_") or k.startswith("k_dcdrift_gray_")]
    for name in names:
        jpeg = coef_jpeg_for(name)
        for pt, opt in ((J.RGB565_LE, 0), (J.RGB565_BE, J.SCALE_HALF), (J.GRAY8, J.SCALE_QUARTER), (J.RGB565_LE, J.SCALE_EIGHTH)):
            rc, got, g = J.decode_to_host(gpu_ctx, jpeg, pt, opt)
            r = ref_scalar.decode_cb(jpeg, pt, opt)
            assert rc == 0 and r["rc"] == 1, (name, pt, opt)
            want = r["canvas"][: g["out_h"], : g["canvas_w"] * g["bpp"]]
            assert np.array_equal(got[: g["out_h"]], want), (name, pt, opt)


@pytest.mark.parametrize("name", sorted(COEF_CASES))
def test_device_prescan(name, gpu_ctx, oracle):
    """the index made on the GPU equals the serial one entry for entry, or -- a predictor past int16 -- the image went to the
    serial pre-scan; either way the pixels are the oracle's"""
    jpeg = coef_jpeg_for(name)
    prep = J.PreparedImage(jpeg, device_prescan=True)
    dimg = J.DeviceImage(gpu_ctx, prep)
    host = J.PreparedImage(jpeg)
    try:
        if _leaves_int16(name):
            assert not dimg.prescan_on_device, name
        elif name not in COEF_CORRUPT:
            assert dimg.prescan_on_device, name
        want_idx, nok = host.block_index()
        got_idx, got_dc = dimg.read_index()
        nb = nok * prep.info.blocks_per_mcu
        assert J.index_equivalent(got_idx[:nb], want_idx[:nb]), name
        assert np.array_equal(got_dc[:nb], host.block_dc()[:nb]), name
        pt = J.GRAY8 if "gray" in name else J.RGB8888
        for opt in (0, J.SCALE_EIGHTH):
            orc, want, _ = oracle.decode_canvas(jpeg, pt, opt)
            g = prep.geometry(pt, opt)
            pitch = (want.shape[1] + 15) // 16 * 16
            out = gpu_ctx.malloc(pitch * want.shape[0])
            b = J.Batch(gpu_ctx, [dimg], [(out, pitch, g["canvas_w"], g["canvas_h"])], [pt], [opt])
            b.decode(); gpu_ctx.sync()
            got = gpu_ctx.to_host(out, pitch * want.shape[0]).reshape(want.shape[0], pitch)[:, : want.shape[1]]
            if orc == 1:
                assert np.array_equal(got, want), (name, opt)
            b.close(); gpu_ctx.free(out)
    finally:
        dimg.close(); host.close(); prep.close()


def test_pipeline_mixes_the_corpus_with_normal_files(gpu_ctx, oracle):
    """one pipeline batch: normal files, the families whose streams the device walks, and the drifted predictors it must hand
    back to the host path"""
    from tests.test_gpu_pipeline import _check, _surfaces
    normal = ["c420_333x217", "c444_333x217", "gray_333x217", "c422_333x217", "c440_200x120"]
    device = [k for k in GOOD if k.startswith(("k_classes_", "k_single_", "k_huff_annexk_", "k_huff_custom_", "k_edge_"))]
    hostp = [k for k in GOOD if _leaves_int16(k) and "_q1" in k]
    names = normal + device + hostp
    jp = [jpeg_for(n) for n in normal] + [coef_jpeg_for(n) for n in device + hostp]
    pts = [J.GRAY8 if "gray" in n else J.RGB8888 for n in names]
    opts = [(0, J.SCALE_HALF, J.SCALE_EIGHTH)[i % 3] for i in range(len(names))]
    pipe = J.Pipeline(gpu_ctx, max_images=len(names), depth=2, host_threads=4)
    outs, metas = _surfaces(gpu_ctx, jp, pts, opts)
    st = pipe.wait(pipe.submit(jp, outs, pts, opts))
    _check(gpu_ctx, oracle, jp, pts, opts, outs, metas, st, names)
    for o in outs:
        gpu_ctx.free(o[0])
    s = pipe.stats
    assert s["images"] == len(names) and s["failed_images"] == 0, s
    assert s["device_images"] == len(normal) + len(device), s
    assert s["host_path_images"] == len(hostp), s
    pipe.close()


def test_p1_in_chunks(gpu_ctx, oracle):
    """P1's chunked mode asked for on every image (JDA_PREPARE_CONT_ALWAYS): the long blocks of the corpus shared out by
    continuation entries"""
    for name in GOOD:
        jpeg = coef_jpeg_for(name)
        p = J.PreparedImage(jpeg, flags=J.PREPARE_CONT_ALWAYS)
        try:
            for pt, opt in ((J.GRAY8, 0),) if "gray" in name else ((J.RGB8888, 0), (J.RGB565_BE, J.SCALE_HALF)):
                st, got, g = J.decode_resident(gpu_ctx, p, pt, opt)
                orc, want, err = oracle.decode_canvas(jpeg, pt, opt)
                assert (st == 0) == (orc == 1), (name, pt, opt, st, orc)
                assert np.array_equal(got, want), (name, pt, opt, int(np.count_nonzero(got != want)))
        finally:
            p.close()


@pytest.mark.parametrize("name", sorted(RUNONLY_CASES))
def test_run_symbols_without_magnitude_bits(name, gpu_ctx, oracle):
    """AC symbols with a run of 1 .. 14 and no value (tests/cases.py, RUNONLY_CASES): nothing is stored for them, in every pixel type and
    scale -- the 1/4-scale kernel stored the stream's next bits as coefficients 8 and 9, which only the GPU showed"""
    jpeg = coef_jpeg_for(name)
    for pt, opt in all_modes(name):
        orc, want, err = oracle.decode_canvas(jpeg, pt, opt)
        rc, got, g = J.decode_to_host(gpu_ctx, jpeg, pt, opt)
        assert orc == 1 and rc == 0, (name, pt, opt, rc, orc, err)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "%s pt=%d opt=%d: %d differing bytes" % (name, pt, opt, int(np.count_nonzero(got != want)))
