"""Host prepare time (parse + filter + pre-scan, no GPU): prepare_time.py file.jpg..  Per file the median of 300 calls under the serial
pre-scan, under the parallel forms asked for by name, and under flags 0 (the library's choice).  JDA_LIBRARY selects the build."""
import sys, time, os, statistics
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "."))
import jpegdec_amd as J
for path in sys.argv[1:] or ["tests/golden/ref/tulips.jpg"]:
    j = open(path, "rb").read()
    for name, flags in (("serial", J.PREPARE_SERIAL_PRESCAN), ("parallel", J.PREPARE_PARALLEL_PRESCAN), ("default", 0)):
        for _ in range(20): J.PreparedImage(j, flags=flags).close()
        us = []
        for _ in range(300):
            t = time.perf_counter()
            im = J.PreparedImage(j, flags=flags)
            us.append((time.perf_counter() - t) * 1e6)
            im.close()
        print("%s %s %.1f us" % (os.path.basename(path), name, statistics.median(us)))
