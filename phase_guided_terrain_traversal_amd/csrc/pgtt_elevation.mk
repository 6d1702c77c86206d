# libpgtt_elevation.so (include/pgtt_elevation.h): the depth-fused elevation map, hand-written HIP for gfx950, one translation unit.
#   make -f pgtt_elevation.mk
# A library of its own: csrc/Makefile, libpgtt.so, the other side libraries and the source hashes they embed are not touched by this file.
# An experiment build names its flavor and goes elsewhere (it is not shipped):
#   make -f pgtt_elevation.mk EXTRA='-DPGTT_ELEVATION_FLAVOR=\"trial\"' BUILD=build/elevation_trial ELEVATION_OUT=build/elevation_trial/libpgtt_elevation_trial.so build/elevation_trial/libpgtt_elevation_trial.so
HIPCC ?= hipcc
ARCH ?= gfx950
BUILD ?= build/elevation
EXTRA ?=
ELEVATION_OUT ?= ../libpgtt_elevation.so
ELEVATION_HDR = pgtt_raycast_host.h ../../include/pgtt_elevation.h ../../include/pgtt_render.h ../../include/pgtt.h
# pgtt_elevation_build_info(): "src=<srchash.side_sha256("elevation"): the unit's include closure, comments and white space removed>;flavor=..."
ELEVATION_FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value -DPGTT_ELEVATION_SRC=\"$(shell python3 ../srchash.py elevation)\" $(EXTRA)

all: $(ELEVATION_OUT)

.PHONY: all clean resources

$(ELEVATION_OUT): $(BUILD)/elevation.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(BUILD)/elevation.o: pgtt_elevation.hip $(ELEVATION_HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(ELEVATION_FLAGS) -c $< -o $@

# per-kernel VGPR / SGPR / scratch / LDS / occupancy report of the device code (no GPU needed)
resources:
	@mkdir -p $(BUILD)
	$(HIPCC) $(ELEVATION_FLAGS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c pgtt_elevation.hip -o $(BUILD)/elevation_resources.o

clean:
	rm -rf $(BUILD) $(ELEVATION_OUT)
