# libpgtt_render.so (include/pgtt_render.h) and libpgtt_depth.so (include/pgtt_depth.h): the two ray-casting side libraries, hand-written HIP
# for gfx950, one translation unit each over the shared pgtt_raycast.hip.h (device algebra) / pgtt_raycast_host.h (host side).
#   make -f pgtt_raycast.mk -j8
# Libraries of their own: csrc/Makefile, libpgtt.so and the source hash pgtt_build_info() embeds are not touched by this file.
# Experiment build of the depth camera with the per-env cull switched off (DESIGN.md 14 quotes its time; it is not shipped):
#   make -f pgtt_raycast.mk EXTRA=-DPGTT_DEPTH_NOCULL BUILD=build/depth_nocull DEPTH_OUT=build/depth_nocull/libpgtt_depth_nocull.so build/depth_nocull/libpgtt_depth_nocull.so
HIPCC ?= hipcc
ARCH ?= gfx950
BUILD ?= build/raycast
EXTRA ?=
RENDER_OUT ?= ../libpgtt_render.so
DEPTH_OUT ?= ../libpgtt_depth.so
CORE = pgtt_raycast.hip.h pgtt_raycast_host.h
RENDER_HDR = $(CORE) ../../include/pgtt_render.h ../../include/pgtt.h
DEPTH_HDR = $(RENDER_HDR) ../../include/pgtt_depth.h
# pgtt_render_build_info() / pgtt_depth_build_info(): "src=<srchash.side_sha256: the unit's include closure, comments and white space removed>;flavor=..."
FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value
RENDER_FLAGS = $(FLAGS) -DPGTT_RENDER_SRC=\"$(shell python3 ../srchash.py render)\"
DEPTH_FLAGS = $(FLAGS) -DPGTT_DEPTH_SRC=\"$(shell python3 ../srchash.py depth)\" $(EXTRA)

all: $(RENDER_OUT) $(DEPTH_OUT)

.PHONY: all clean resources

$(RENDER_OUT): $(BUILD)/render.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(DEPTH_OUT): $(BUILD)/depth.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(BUILD)/render.o: pgtt_render.hip $(RENDER_HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(RENDER_FLAGS) -c $< -o $@

$(BUILD)/depth.o: pgtt_depth.hip $(DEPTH_HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(DEPTH_FLAGS) -c $< -o $@

# per-kernel VGPR / SGPR / scratch / occupancy report of the device code of both libraries (no GPU needed)
resources:
	@mkdir -p $(BUILD)
	$(HIPCC) $(RENDER_FLAGS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c pgtt_render.hip -o $(BUILD)/render_resources.o
	$(HIPCC) $(DEPTH_FLAGS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c pgtt_depth.hip -o $(BUILD)/depth_resources.o

clean:
	rm -rf $(BUILD) $(RENDER_OUT) $(DEPTH_OUT)
