# libpgtt_render.so: the batched ray-cast renderer (include/pgtt_render.h), hand-written HIP for gfx950.
#   make -f pgtt_render.mk -j8
# A library of its own: csrc/Makefile, libpgtt.so and the source hash pgtt_build_info() embeds are not touched by it.
HIPCC ?= hipcc
ARCH ?= gfx950
BUILD ?= build/render
OUT ?= ../libpgtt_render.so
HDR = ../../include/pgtt_render.h ../../include/pgtt.h
# pgtt_render_build_info(): "src=<SHA-256 of pgtt_render.hip and pgtt_render.h>;flavor=product"
RENDER_SRCHASH := $(shell cat pgtt_render.hip ../../include/pgtt_render.h | sha256sum | cut -c1-64)
FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value -DPGTT_RENDER_SRC=\"$(RENDER_SRCHASH)\"

all: $(OUT)

.PHONY: all clean resources

$(OUT): $(BUILD)/render.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(BUILD)/render.o: pgtt_render.hip $(HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(FLAGS) -c $< -o $@

# per-kernel VGPR / SGPR / scratch / occupancy report of the device code (no GPU needed)
resources: pgtt_render.hip $(HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(FLAGS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c $< -o $(BUILD)/render_resources.o

clean:
	rm -rf $(BUILD) $(OUT)
