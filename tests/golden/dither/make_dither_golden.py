"""Generator of tests/golden/dither: the canvases made for the dither tests (*.jpg) and dither_golden.json -- for every case of
tests/ref_dither.py the draw log and a digest of the packed rows the UNMODIFIED reference's decodeDither hands to its draw callback
(oracle/_ref/libjpegdec_ref_scalar.so, built from the reference tree by oracle/Makefile; driven by tests/ref_dither.py).

    python tests/golden/dither/make_dither_golden.py

Small files: digests, not images.  The tests hold the product, its host simulator and -- where oracle/_ref exists -- the live
reference to these."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from jpegdec_amd.synth import synth_jpeg  # noqa: E402
from tests import ref_dither as R  # noqa: E402


def main():
    assert R.available(), "build oracle/_ref first (make -C oracle ref)"
    os.makedirs(R.DITHER_DIR, exist_ok=True)
    for name, kw in list(R.SIM_JPEGS.items()) + list(R.NO_REFERENCE_JPEGS.items()):
        path = os.path.join(R.DITHER_DIR, name + ".jpg")
        if not os.path.exists(path):
            open(path, "wb").write(synth_jpeg(**kw))
    out = {}
    for name, pt, opt in R.recorded_cases():
        rc, err, log, strips = R.ref_decode_dither(R.any_jpeg(name), pt, opt)
        assert rc == 1 and err == 0, (name, pt, opt, rc, err)
        out[R.case_key(name, pt, opt)] = R.digest(log, R.clip_strips(strips, log))
    # the same image at an offset, and with a callback that stops the decode after two strips
    for name in ("c420_333x217", "gray_333x217"):
        for pt in R.DITHER_TYPES:
            rc, err, log, strips = R.ref_decode_dither(R.any_jpeg(name), pt, 0, xy=(3, 5))
            assert rc == 1
            out[R.case_key(name, pt, 0) + ":xy3,5"] = R.digest(log, R.clip_strips(strips, log))
            rc, err, log, strips = R.ref_decode_dither(R.any_jpeg(name), pt, 2, stop_after=2)
            out[R.case_key(name, pt, 2) + ":stop2"] = dict(R.digest(log, R.clip_strips(strips, log)), rc=rc, err=err)
    for pt in R.DITHER_TYPES:                            # the EXIF thumbnail of a file (its header parsed over the main image's)
        rc, err, log, strips = R.ref_decode_dither(R.exif_thumbnail_jpeg(), pt, R.JPEG_EXIF_THUMBNAIL)
        assert rc == 1 and err == 0 and log[0][2] == 72, (rc, err, log[:1])
        out["exifthumb:%d" % pt] = R.digest(log, R.clip_strips(strips, log))
    json.dump(out, open(R.GOLDEN, "w"), indent=0, sort_keys=True)
    print("%d cases -> %s" % (len(out), R.GOLDEN))


if __name__ == "__main__":
    main()
