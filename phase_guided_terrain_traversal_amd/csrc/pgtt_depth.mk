# libpgtt_depth.so: the onboard depth camera (include/pgtt_depth.h), hand-written HIP for gfx950.
#   make -f pgtt_depth.mk -j8
# A library of its own: csrc/Makefile, pgtt_render.mk, libpgtt.so, libpgtt_render.so and the source hashes they embed are not touched by it.
# Experiment build with the per-env cull switched off (DESIGN.md 14 quotes its time; it is not shipped):
#   make -f pgtt_depth.mk EXTRA=-DPGTT_DEPTH_NOCULL BUILD=build/depth_nocull OUT=build/depth_nocull/libpgtt_depth_nocull.so
HIPCC ?= hipcc
ARCH ?= gfx950
BUILD ?= build/depth
OUT ?= ../libpgtt_depth.so
EXTRA ?=
HDR = ../../include/pgtt_depth.h ../../include/pgtt_render.h ../../include/pgtt.h
# pgtt_depth_build_info(): "src=<SHA-256 of pgtt_depth.hip and pgtt_depth.h>;flavor=product"
DEPTH_SRCHASH := $(shell cat pgtt_depth.hip ../../include/pgtt_depth.h | sha256sum | cut -c1-64)
FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value -DPGTT_DEPTH_SRC=\"$(DEPTH_SRCHASH)\" $(EXTRA)

all: $(OUT)

.PHONY: all clean resources

$(OUT): $(BUILD)/depth.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(BUILD)/depth.o: pgtt_depth.hip $(HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(FLAGS) -c $< -o $@

# per-kernel VGPR / SGPR / scratch / occupancy report of the device code (no GPU needed)
resources: pgtt_depth.hip $(HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(FLAGS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c $< -o $(BUILD)/depth_resources.o

clean:
	rm -rf $(BUILD) $(OUT)
