# Top-level build.  `make` builds everything that can be built where it runs:
#   jpegdec_amd/libjpegdec_amd.so   the product: host front end + HIP runtime + gfx950 kernels (hipcc)
#   oracle/liboracle.so             the checker (CPU restatement)            -- test infrastructure
#   oracle/_ref/*.so                the real reference, if /root/reference is present -- test infrastructure
#   tests/hostsim/libjda_hostsim.so wave emulator for CPU-only unit tests    -- test infrastructure
# and on request: `make devprims` (tests/devprims/libjda_devprims.so: both sides of every device-only helper branch, hipcc) and
# `make devprimsasan` (tests/devprims/devprims_asan: their host sides as a program under ASan + UBSan) -- test infrastructure
HIPCC ?= /opt/rocm/bin/hipcc
CXX   ?= g++
ARCH  ?= gfx950
CSRC  = jpegdec_amd/csrc
EXTRA ?=
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -shared -fwrapv -pthread -Wall -Wno-unused-function -Xarch_host -ffp-contract=off -Iinclude $(EXTRA)
LIB = jpegdec_amd/libjpegdec_amd.so
LIB_SRCS = $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp $(CSRC)/jda_runtime.cpp $(CSRC)/jda_encode_progressive.cpp $(CSRC)/jda_pipeline.cpp $(CSRC)/jda_node.cpp $(CSRC)/jda_kernels.hip $(CSRC)/JPEGDEC.cpp
LIB_DEPS = $(LIB_SRCS) $(CSRC)/jda_runtime_internal.h $(CSRC)/jda_internal.h $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_pack_plan.h $(CSRC)/jda_unpack_plan.h $(CSRC)/jda_exact_plan.h $(CSRC)/jda_resize_plan.h $(CSRC)/jda_reduce_plan.h $(CSRC)/jda_thumbnail_plan.h $(CSRC)/jda_encode_plan.h $(CSRC)/jda_encode_prog_plan.h $(CSRC)/jda_recode_plan.h $(CSRC)/jda_prescan_plan.h include/jpegdec_amd.h include/JPEGDEC.h

all: lib oracle hostsim classshim

lib: $(LIB)
$(LIB): $(LIB_DEPS)
	$(HIPCC) $(HIPFLAGS) -o $@ $(LIB_SRCS)

oracle:
	$(MAKE) -C oracle all

hostsim: tests/hostsim/libjda_reducesim.so tests/hostsim/libjda_exactrectsim.so tests/hostsim/libjda_exactadobesim.so tests/hostsim/libjda_exactscaledsim.so tests/hostsim/libjda_exactsim.so tests/hostsim/libjda_hostsim.so tests/hostsim/libjda_dithersim.so tests/hostsim/libjda_orientsim.so tests/hostsim/libjda_coefsim.so tests/hostsim/libjda_packsim.so tests/hostsim/libjda_resizesim.so tests/hostsim/libjda_coefsparsesim.so tests/hostsim/libjda_encodesim.so tests/hostsim/libjda_huffoptsim.so tests/hostsim/libjda_resizefilterssim.so tests/hostsim/libjda_encodeprogsim.so tests/hostsim/libjda_recodesim.so tests/hostsim/libjda_recodexfsim.so tests/hostsim/libjda_unpacksim.so
tests/hostsim/libjda_hostsim.so: tests/hostsim/hostsim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_prescan_plan.h $(CSRC)/jda_internal.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Iinclude -pthread -o $@ tests/hostsim/hostsim.cpp $(CSRC)/jda_frontend.cpp

# the dither kernel's lane schedule and its row-major twin on the CPU (tests/test_dither_cpu.py) -- test infrastructure
tests/hostsim/libjda_dithersim.so: tests/hostsim/dither_sim.cpp tests/hostsim/dither_twin.h $(CSRC)/jda_frontend.cpp $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/dither_sim.cpp $(CSRC)/jda_frontend.cpp

# the orient kernel's tile schedule, lane by lane, and its row-major twin on the CPU (tests/test_orient_cpu.py) -- test infrastructure
tests/hostsim/libjda_orientsim.so: tests/hostsim/orient_sim.cpp tests/hostsim/orient_twin.h $(CSRC)/jda_frontend.cpp $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/orient_sim.cpp $(CSRC)/jda_frontend.cpp

# the coefficient-tile kernel's lane schedule and its row-major twin on the CPU (tests/test_progressive_full_cpu.py) -- test infrastructure
tests/hostsim/libjda_coefsim.so: tests/hostsim/coef_sim.cpp tests/hostsim/coef_twin.h $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/coef_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp

# the sparse coefficient form and the load phase of jda_sparse_tiles, lane by lane, against the dense load phase (tests/test_sparse_coef_cpu.py) -- test infrastructure
COEFSPARSE_SRCS = tests/hostsim/coef_sparse_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp
COEFSPARSE_DEPS = $(COEFSPARSE_SRCS) $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_coefsparsesim.so: $(COEFSPARSE_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ $(COEFSPARSE_SRCS)
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
sparsepack: tests/hostsim/sparse_pack_asan
tests/hostsim/sparse_pack_asan: tests/hostsim/sparse_pack_main.cpp $(COEFSPARSE_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/sparse_pack_main.cpp $(COEFSPARSE_SRCS)

# the pack kernel's vector schedule, lane by lane, its row-major twin and the argument checks of jda_pack_surfaces on the CPU (tests/test_pack_cpu.py) -- test infrastructure
tests/hostsim/libjda_packsim.so: tests/hostsim/pack_sim.cpp tests/hostsim/pack_twin.h $(CSRC)/jda_pack_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/pack_sim.cpp

# the unpack kernel's vector schedule, lane by lane, its row-major twin and the argument checks of jda_unpack_surfaces on the CPU
# (tests/test_unpack_cpu.py) -- test infrastructure.  -ffp-contract=off: a float element is a product rounded, then a sum rounded
UNPACKSIM_DEPS = tests/hostsim/unpack_sim.cpp tests/hostsim/unpack_twin.h $(CSRC)/jda_unpack_plan.h $(CSRC)/jda_pack_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_unpacksim.so: $(UNPACKSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -ffp-contract=off -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/unpack_sim.cpp
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
unpackasan: tests/hostsim/unpack_asan
tests/hostsim/unpack_asan: tests/hostsim/unpack_main.cpp $(UNPACKSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/unpack_main.cpp tests/hostsim/unpack_sim.cpp

# the exact decode's kernels lane by lane over the runtime's plan, and their row-major twin, on the CPU (tests/test_exact_cpu.py) -- test infrastructure
EXACTSIM_SRCS = tests/hostsim/exact_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp
EXACTSIM_DEPS = $(EXACTSIM_SRCS) tests/hostsim/exact_twin.h $(CSRC)/jda_exact_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_exactsim.so: $(EXACTSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ $(EXACTSIM_SRCS)
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
exactasan: tests/hostsim/exact_asan
tests/hostsim/exact_asan: tests/hostsim/exact_main.cpp $(EXACTSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/exact_main.cpp $(EXACTSIM_SRCS)

# the scaled exact decode's kernels (1/2, 1/4, 1/8) lane by lane, and their row-major twin, on the CPU (tests/test_exact_scaled_cpu.py) -- test infrastructure
EXACTSCALEDSIM_SRCS = tests/hostsim/exact_scaled_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp
EXACTSCALEDSIM_DEPS = $(EXACTSCALEDSIM_SRCS) tests/hostsim/exact_scaled_twin.h tests/hostsim/exact_twin.h $(CSRC)/jda_exact_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_exactscaledsim.so: $(EXACTSCALEDSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ $(EXACTSCALEDSIM_SRCS)
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
exactscaledasan: tests/hostsim/exact_scaled_asan
tests/hostsim/exact_scaled_asan: tests/hostsim/exact_scaled_main.cpp $(EXACTSCALEDSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/exact_scaled_main.cpp $(EXACTSCALEDSIM_SRCS)

# the colour models of the exact decode (Adobe, RGB-coded, CMYK, YCCK): jda_exact_colour4 and the RGB colour instances lane by lane over the
# runtime's plan and the host scan decoder's coefficient images, and their row-major twin, on the CPU (tests/test_exact_adobe_cpu.py) -- test infrastructure
EXACTADOBESIM_SRCS = tests/hostsim/exact_adobe_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp
EXACTADOBESIM_DEPS = $(EXACTADOBESIM_SRCS) tests/hostsim/exact_twin.h $(CSRC)/jda_exact_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_exactadobesim.so: $(EXACTADOBESIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ $(EXACTADOBESIM_SRCS)
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
exactadobeasan: tests/hostsim/exact_adobe_asan
tests/hostsim/exact_adobe_asan: tests/hostsim/exact_adobe_main.cpp $(EXACTADOBESIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/exact_adobe_main.cpp $(EXACTADOBESIM_SRCS)

# the exact decode of a pixel rectangle: the plan, the existing planes lanes over the rectangle's tiles into a poisoned scratch and the new
# colour lanes (jda_exr_*) lane by lane on the CPU (tests/test_exact_rect_cpu.py) -- test infrastructure
EXACTRECTSIM_SRCS = tests/hostsim/exact_rect_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp
EXACTRECTSIM_DEPS = $(EXACTRECTSIM_SRCS) tests/hostsim/exact_scaled_twin.h tests/hostsim/exact_twin.h $(CSRC)/jda_exact_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_plan.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_exactrectsim.so: $(EXACTRECTSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ $(EXACTRECTSIM_SRCS)
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
exactrectasan: tests/hostsim/exact_rect_asan
tests/hostsim/exact_rect_asan: tests/hostsim/exact_rect_main.cpp $(EXACTRECTSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/exact_rect_main.cpp $(EXACTRECTSIM_SRCS)

# the resize kernel's two passes, lane by lane, its row-major twin, the host's tap tables and the argument checks of jda_resize_surfaces on
# the CPU (tests/test_resize_cpu.py) -- test infrastructure.  -ffp-contract=off: the taps are Pillow's only in Pillow's order of operations
tests/hostsim/libjda_resizesim.so: tests/hostsim/resize_sim.cpp tests/hostsim/resize_twin.h $(CSRC)/jda_resize_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -ffp-contract=off -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/resize_sim.cpp

# the same for Pillow's five filters through jda_resize_surfaces_ex's plan and the signed instances of the two passes
# (tests/test_resize_filters_cpu.py) -- test infrastructure; resize_filters_sim.cpp includes resize_sim.cpp for its memory policy
RESIZEFSIM_DEPS = tests/hostsim/resize_filters_sim.cpp tests/hostsim/resize_sim.cpp tests/hostsim/resize_twin.h $(CSRC)/jda_resize_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_resizefilterssim.so: $(RESIZEFSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -ffp-contract=off -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/resize_filters_sim.cpp
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
resizefiltersasan: tests/hostsim/resize_filters_asan
tests/hostsim/resize_filters_asan: tests/hostsim/resize_filters_main.cpp $(RESIZEFSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/resize_filters_main.cpp tests/hostsim/resize_filters_sim.cpp

# the reduce kernel's two phases, lane by lane, the argument checks of jda_reduce_surfaces and jda_resize_surfaces_box, the tap tables of
# fractional boxes and the thumbnail plan on the CPU (tests/test_thumbnail_cpu.py) -- test infrastructure.  -ffp-contract=off: the taps and
# the plan are Pillow's only in Pillow's order of operations
REDUCESIM_DEPS = tests/hostsim/reduce_sim.cpp $(CSRC)/jda_thumbnail_plan.h $(CSRC)/jda_reduce_plan.h $(CSRC)/jda_resize_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_reducesim.so: $(REDUCESIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -ffp-contract=off -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/reduce_sim.cpp
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
thumbasan: tests/hostsim/thumb_asan
tests/hostsim/thumb_asan: tests/hostsim/thumb_main.cpp $(REDUCESIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/thumb_main.cpp tests/hostsim/reduce_sim.cpp

# the encode kernels' six stages, lane by lane, the header builder and the argument checks of jda_encode_surfaces on the CPU
# (tests/test_encode_cpu.py) -- test infrastructure
ENCODESIM_DEPS = tests/hostsim/encode_sim.cpp $(CSRC)/jda_encode_plan.h $(CSRC)/jda_device_core.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
tests/hostsim/libjda_encodesim.so: $(ENCODESIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/encode_sim.cpp
# .. and the same with a main of its own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
encodeasan: tests/hostsim/encode_asan
tests/hostsim/encode_asan: tests/hostsim/encode_main.cpp $(ENCODESIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/encode_main.cpp tests/hostsim/encode_sim.cpp

# the nine stages of a call with optimised jobs (jda_encode_surfaces_ex, JDA_ENCODE_OPTIMIZE), lane by lane, and the table builder on the CPU
# (tests/test_encode_opt_cpu.py) -- test infrastructure; huffopt_sim.cpp includes encode_sim.cpp for its memory policy
HUFFOPTSIM_DEPS = tests/hostsim/huffopt_sim.cpp $(ENCODESIM_DEPS)
tests/hostsim/libjda_huffoptsim.so: $(HUFFOPTSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/huffopt_sim.cpp
huffoptasan: tests/hostsim/huffopt_asan
tests/hostsim/huffopt_asan: tests/hostsim/huffopt_main.cpp $(HUFFOPTSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/huffopt_main.cpp tests/hostsim/huffopt_sim.cpp

# the progressive encode's plan and stages (jda_encode_prog_plan.h, jda_pe_* of jda_device_core.h) as a library for the CPU tests
# (tests/test_encode_prog_cpu.py) and as a program of its own under ASan + UBSan -- test infrastructure
ENCODEPROGSIM_DEPS = tests/hostsim/encode_prog_sim.cpp $(CSRC)/jda_encode_prog_plan.h $(ENCODESIM_DEPS)
tests/hostsim/libjda_encodeprogsim.so: $(ENCODEPROGSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/encode_prog_sim.cpp
encodeprogasan: tests/hostsim/encode_prog_asan
tests/hostsim/encode_prog_asan: tests/hostsim/encode_prog_main.cpp $(ENCODEPROGSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/encode_prog_main.cpp tests/hostsim/encode_prog_sim.cpp

# the recode plan and its two stages (jda_recode_plan.h, jda_rc_* of jda_device_core.h) over sources the product's front end prepares, as a
# library for the CPU tests (tests/test_recode_cpu.py) and as a program of its own under ASan + UBSan -- test infrastructure
RECODESIM_SRCS = tests/hostsim/recode_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp
RECODESIM_DEPS = $(RECODESIM_SRCS) $(CSRC)/jda_recode_plan.h $(CSRC)/jda_encode_prog_plan.h $(CSRC)/jda_plan.h $(ENCODESIM_DEPS)
tests/hostsim/libjda_recodesim.so: $(RECODESIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ $(RECODESIM_SRCS)
recodeasan: tests/hostsim/recode_asan
tests/hostsim/recode_asan: tests/hostsim/recode_main.cpp $(RECODESIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/recode_main.cpp $(RECODESIM_SRCS)

# the same with a flip, a turn, a transposition or an MCU crop a job (jda_recode_images_ex's plan, jda_rc_*_xf of jda_device_core.h), as a
# library for the CPU tests (tests/test_recode_xf_cpu.py) and as a program of its own under ASan + UBSan -- test infrastructure;
# recode_xf_sim.cpp includes recode_sim.cpp for its sources, its memory policy and the stages behind
RECODEXFSIM_SRCS = tests/hostsim/recode_xf_sim.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp
RECODEXFSIM_DEPS = $(RECODEXFSIM_SRCS) $(RECODESIM_DEPS)
tests/hostsim/libjda_recodexfsim.so: $(RECODEXFSIM_DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fwrapv -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ $(RECODEXFSIM_SRCS)
recodexfasan: tests/hostsim/recode_xf_asan
tests/hostsim/recode_xf_asan: tests/hostsim/recode_xf_main.cpp $(RECODEXFSIM_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/hostsim/recode_xf_main.cpp $(RECODEXFSIM_SRCS)

# both sides of every `#if defined(__HIP_DEVICE_COMPILE__)` fork of jda_device_core.h behind one C interface: the helpers' host sides in a loop,
# their device sides in a plain kernel, built with the product's HIPFLAGS flag for flag (tests/test_devprims_cpu.py, tests/test_gpu_devprims.py)
# -- test infrastructure
DEVPRIMS_DEPS = tests/devprims/devprims_ops.h $(CSRC)/jda_device_core.h $(CSRC)/jda_internal.h include/jpegdec_amd.h
devprims: tests/devprims/libjda_devprims.so
tests/devprims/libjda_devprims.so: tests/devprims/devprims.hip $(DEVPRIMS_DEPS)
	$(HIPCC) $(HIPFLAGS) -o $@ tests/devprims/devprims.hip
# .. and the host sides with a main of their own under AddressSanitizer + UBSan: a program, nothing loaded into an interpreter
devprimsasan: tests/devprims/devprims_asan
tests/devprims/devprims_asan: tests/devprims/devprims_main.cpp $(DEVPRIMS_DEPS)
	$(CXX) -O1 -g -std=c++17 -fwrapv -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes -Iinclude -pthread -o $@ tests/devprims/devprims_main.cpp

# the reference-API driver (oracle/ref_shim.cpp) built against the product's JPEGDEC class -- test infrastructure
classshim: tests/libjpegdec_class_shim.so
tests/libjpegdec_class_shim.so: oracle/ref_shim.cpp include/JPEGDEC.h $(LIB)
	$(CXX) -O2 -std=c++17 -fPIC -shared -w -DSHIM_PRODUCT -Iinclude -o $@ oracle/ref_shim.cpp -Ljpegdec_amd -ljpegdec_amd -lpthread -Wl,-rpath,'$$ORIGIN/../jpegdec_amd'

# the same driver over the class's HOST logic alone: JPEGDEC.cpp + the host front end + a CPU stand-in for the device entry points
# (tests/class_cpu/stub_runtime.cpp: pixels from the oracle) -- test infrastructure: the recorded reference walks run on it without a
# GPU (tests/test_class_walks_cpu.py), the second build under AddressSanitizer
classcpu: tests/class_cpu/libjpegdec_class_cpu.so tests/class_cpu/walks_asan
CLASS_CPU_SRCS = oracle/ref_shim.cpp $(CSRC)/JPEGDEC.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_progressive.cpp tests/class_cpu/stub_runtime.cpp tests/class_cpu/stub_dither.cpp tests/class_cpu/stub_orient.cpp tests/class_cpu/stub_coef.cpp
tests/class_cpu/libjpegdec_class_cpu.so: $(CLASS_CPU_SRCS) tests/hostsim/dither_twin.h tests/hostsim/orient_twin.h tests/hostsim/coef_twin.h oracle/jpegdec_oracle.c include/JPEGDEC.h include/jpegdec_amd.h
	$(CC) -O2 -std=c11 -fPIC -c -o tests/class_cpu/oracle.o oracle/jpegdec_oracle.c
	$(CXX) -O2 -std=c++17 -fPIC -shared -w -DSHIM_PRODUCT -Iinclude -o $@ $(CLASS_CPU_SRCS) tests/class_cpu/oracle.o -lpthread
tests/class_cpu/walks_asan: $(CLASS_CPU_SRCS) tests/hostsim/dither_twin.h tests/hostsim/orient_twin.h tests/hostsim/coef_twin.h tests/class_cpu/walks_main.cpp oracle/jpegdec_oracle.c include/JPEGDEC.h include/jpegdec_amd.h
	$(CC) -O1 -g -std=c11 -fsanitize=address,undefined -fno-omit-frame-pointer -c -o tests/class_cpu/oracle_asan.o oracle/jpegdec_oracle.c
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -w -DSHIM_PRODUCT -Iinclude -o $@ $(CLASS_CPU_SRCS) tests/class_cpu/walks_main.cpp tests/class_cpu/oracle_asan.o -lpthread

# a plain C program on the C flavour of the API (JPEG_openFile / JPEG_decode / ...), compiled with the C compiler
cuser: tests/capi_c/c_user
tests/capi_c/c_user: tests/capi_c/c_user.c include/JPEGDEC.h $(LIB)
	$(CC) -std=c99 -O2 -Wall -Iinclude -o $@ tests/capi_c/c_user.c -Ljpegdec_amd -ljpegdec_amd -Wl,-rpath,'$$ORIGIN/../../jpegdec_amd'

# a plain C program decoding with a caller-chosen option word (JPEG_PROGRESSIVE_FULL: tests/test_gpu_progressive_full.py)
proguser: tests/capi_c/prog_user
tests/capi_c/prog_user: tests/capi_c/prog_user.c include/JPEGDEC.h $(LIB)
	$(CC) -std=c99 -O2 -Wall -Iinclude -o $@ tests/capi_c/prog_user.c -Ljpegdec_amd -ljpegdec_amd -Wl,-rpath,'$$ORIGIN/../../jpegdec_amd'

# a plain C program on the node entry points (jda_node_*): one file decoded n times over every GPU of the node
nodeuser: tests/capi_c/node_user
tests/capi_c/node_user: tests/capi_c/node_user.c include/jpegdec_amd.h $(LIB)
	$(CC) -std=c99 -O2 -Wall -Iinclude -o $@ tests/capi_c/node_user.c -Ljpegdec_amd -ljpegdec_amd -Wl,-rpath,'$$ORIGIN/../../jpegdec_amd'

# the reference's jpeg_perf_test (examples/jpeg_perf_test/jpeg_perf_test.ino) as a C program on the product library: bench.py's c1 leg
perfuser: tests/capi_c/perf_user
tests/capi_c/perf_user: tests/capi_c/perf_user.c include/JPEGDEC.h $(LIB)
	$(CC) -std=c99 -O2 -Wall -Iinclude -o $@ tests/capi_c/perf_user.c -Ljpegdec_amd -ljpegdec_amd -Wl,-rpath,'$$ORIGIN/../../jpegdec_amd'

# the boundary's object semantics (class copies / moves, JPEGIMAGE without initialisation or close) -- opens only, no GPU needed
semuser: tests/capi_c/semantics_user
tests/capi_c/semantics_user: tests/capi_c/semantics_user.cpp include/JPEGDEC.h $(LIB)
	$(CXX) -std=c++17 -O2 -Wall -Iinclude -o $@ tests/capi_c/semantics_user.cpp -Ljpegdec_amd -ljpegdec_amd -Wl,-rpath,'$$ORIGIN/../../jpegdec_amd'

# the reference's own test program (MacOS/JPEGDEC_Test/JPEGDEC_Test/main.cpp) restated against the product's class
jpegtest: tests/ref_main/jpegtest_amd
tests/ref_main/jpegtest_amd: tests/ref_main/jpegtest_amd.cpp include/JPEGDEC.h $(LIB)
	$(CXX) -std=c++17 -O2 -Wall -Iinclude -o $@ tests/ref_main/jpegtest_amd.cpp -Ljpegdec_amd -ljpegdec_amd -Wl,-rpath,'$$ORIGIN/../../jpegdec_amd'

# the host front end under ASan + UBSan with a mutation driver (no GPU code in jda_frontend.cpp)
frontfuzz: tests/fuzz/frontend_fuzz
tests/fuzz/frontend_fuzz: tests/fuzz/frontend_fuzz.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -Wall -Iinclude -pthread -o $@ tests/fuzz/frontend_fuzz.cpp $(CSRC)/jda_frontend.cpp

# the same driver under ThreadSanitizer: the interval-parallel host pre-scan (helper threads, jda_frontend.cpp) over restart streams
chunkequiv: tests/fuzz/chunk_equiv
tests/fuzz/chunk_equiv: tests/fuzz/chunk_equiv.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -DJDA_TEST_CHUNK_BYTES_HOOK -Wall -Iinclude -pthread -o $@ tests/fuzz/chunk_equiv.cpp $(CSRC)/jda_frontend.cpp

fronttsan: tests/fuzz/frontend_tsan
tests/fuzz/frontend_tsan: tests/fuzz/frontend_fuzz.cpp $(CSRC)/jda_frontend.cpp $(CSRC)/jda_internal.h include/jpegdec_amd.h
	$(CXX) -std=c++17 -O1 -g -fsanitize=thread -fno-omit-frame-pointer -Wall -Iinclude -pthread -o $@ tests/fuzz/frontend_fuzz.cpp $(CSRC)/jda_frontend.cpp

clean:
	rm -f tests/devprims/libjda_devprims.so tests/devprims/devprims_asan tests/hostsim/libjda_reducesim.so tests/hostsim/thumb_asan tests/hostsim/libjda_exactrectsim.so tests/hostsim/exact_rect_asan tests/hostsim/libjda_exactadobesim.so tests/hostsim/exact_adobe_asan tests/hostsim/libjda_exactscaledsim.so tests/hostsim/exact_scaled_asan tests/hostsim/libjda_exactsim.so tests/hostsim/exact_asan tests/hostsim/libjda_unpacksim.so tests/hostsim/unpack_asan tests/hostsim/libjda_recodexfsim.so tests/hostsim/recode_xf_asan tests/hostsim/libjda_recodesim.so tests/hostsim/recode_asan tests/hostsim/libjda_encodeprogsim.so tests/hostsim/encode_prog_asan tests/fuzz/frontend_tsan $(LIB) tests/class_cpu/*.so tests/class_cpu/*.o tests/class_cpu/walks_asan tests/fuzz/frontend_fuzz tests/fuzz/chunk_equiv tests/ref_main/jpegtest_amd tests/hostsim/libjda_hostsim.so tests/hostsim/libjda_dithersim.so tests/hostsim/libjda_orientsim.so tests/hostsim/libjda_coefsim.so tests/hostsim/libjda_packsim.so tests/hostsim/libjda_resizesim.so tests/hostsim/libjda_coefsparsesim.so tests/hostsim/sparse_pack_asan tests/hostsim/libjda_encodesim.so tests/hostsim/encode_asan tests/hostsim/libjda_huffoptsim.so tests/hostsim/huffopt_asan tests/hostsim/libjda_resizefilterssim.so tests/hostsim/resize_filters_asan tests/capi_c/c_user tests/capi_c/node_user tests/capi_c/semantics_user tests/capi_c/perf_user tests/capi_c/prog_user
	$(MAKE) -C oracle clean

.PHONY: devprims devprimsasan thumbasan exactrectasan exactadobeasan exactscaledasan exactasan all lib oracle hostsim classshim classcpu sparsepack encodeasan huffoptasan encodeprogasan recodeasan recodexfasan resizefiltersasan unpackasan cuser nodeuser semuser perfuser proguser fronttsan chunkequiv jpegtest frontfuzz nodestub clean

# jda_node.cpp (host code above the C-ABI) over eight pretend devices -- test infrastructure, no GPU (tests/test_c_api.py)
nodestub: tests/node_stub/node_stub_user
tests/node_stub/node_stub_user: tests/node_stub/node_stub_user.cpp tests/node_stub/stub_pipeline.cpp $(CSRC)/jda_node.cpp include/jpegdec_amd.h
	$(CXX) -std=c++17 -O1 -g -fsanitize=thread -Wall -Iinclude -pthread -o $@ tests/node_stub/node_stub_user.cpp tests/node_stub/stub_pipeline.cpp $(CSRC)/jda_node.cpp
