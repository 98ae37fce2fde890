# fft_wgpu_amd/side/side.mk -- the build of one side plan library, included by ../strided, ../fft2d, ../real, ../conv and
# ../stft/Makefile, for gfx950 only.  A side library sits beside csrc/, not in it: its kernels share nothing with the records
# that are stamped with csrc's sources.  Two translation units as in csrc/Makefile: kernels_$(NAME).hip (kernels + launcher,
# compiled as HIP for $(ARCH)) and $(NAME).cpp (the C ABI, plain C++ against the HIP runtime API).  The library links
# against ../libfft_wgpu_amd.so (contexts, buffers, streams, error strings), which it finds beside itself ($ORIGIN) and which
# is built first when it is missing.  The including Makefile sets
#   NAME      the directory: kernels_$(NAME).hip and $(NAME).cpp
#   LIB       the library: ../libfft_wgpu_amd_$(LIB).so
#   HDRS      the headers of its own that both units read (beyond ../csrc/kernels.h and schedule.h)
#   HOST_HDR  the public headers $(NAME).cpp reads (beyond ../../include/fft_wgpu_amd.h)
#   LIBS, DEPS  (optional) side libraries it links against: the -l flags and the files, which need a rule of their own
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
FLAGS     = -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $(EXTRA)
CXXFLAGS  = $(FLAGS) --offload-arch=$(ARCH)
HOSTFLAGS = $(FLAGS) -x c++ -D__HIP_PLATFORM_AMD__ -I$(abspath $(dir $(HIPCC))../include)
OUT       = ../libfft_wgpu_amd_$(LIB).so
MAIN      = ../libfft_wgpu_amd.so
OBJS      = kernels_$(NAME).o $(NAME).o
HDRS     += ../csrc/kernels.h ../csrc/schedule.h
DEV_HDRS  = ../strided/strided_net.h ../csrc/cplx.h ../csrc/device_common.h
HOST_HDR += ../side/side_host.h ../csrc/internal.h ../csrc/handles.h ../../include/fft_wgpu_amd.h

all: $(OUT)
# the objects are intermediate: a tree that holds the library but not its objects is up to date
.SECONDARY: $(OBJS)
$(MAIN):
	$(MAKE) -C ../csrc all
kernels_$(NAME).o: kernels_$(NAME).hip $(HDRS) $(DEV_HDRS)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@
$(NAME).o: $(NAME).cpp $(HDRS) $(HOST_HDR)
	$(HIPCC) $(HOSTFLAGS) -c $< -o $@
$(OUT): $(OBJS) | $(MAIN) $(DEPS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -L.. $(strip $(LIBS) -lfft_wgpu_amd) -Wl,-rpath,'$$ORIGIN'
clean:
	rm -f *.o $(OUT)
