# libpgtt_perceive.so (include/pgtt_perceive.h): the student perception module, hand-written HIP for gfx950, one translation unit.
#   make -f pgtt_perceive.mk
# A library of its own: csrc/Makefile, libpgtt.so and the source hash pgtt_build_info() embeds are not touched by this file.
# An experiment build names its flavor and goes elsewhere (it is not shipped):
#   make -f pgtt_perceive.mk EXTRA='-DPGTT_PERCEIVE_FLAVOR=\"trial\"' BUILD=build/perceive_trial PERCEIVE_OUT=build/perceive_trial/libpgtt_perceive_trial.so build/perceive_trial/libpgtt_perceive_trial.so
HIPCC ?= hipcc
ARCH ?= gfx950
BUILD ?= build/perceive
EXTRA ?=
PERCEIVE_OUT ?= ../libpgtt_perceive.so
PERCEIVE_HDR = pgtt_raycast_host.h ../../include/pgtt_perceive.h ../../include/pgtt_render.h ../../include/pgtt.h
# pgtt_perceive_build_info(): "src=<srchash.side_sha256("perceive"): the unit's include closure, comments and white space removed>;flavor=..."
PERCEIVE_FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value -DPGTT_PERCEIVE_SRC=\"$(shell python3 ../srchash.py perceive)\" $(EXTRA)

all: $(PERCEIVE_OUT)

.PHONY: all clean resources

$(PERCEIVE_OUT): $(BUILD)/perceive.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(BUILD)/perceive.o: pgtt_perceive.hip $(PERCEIVE_HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(PERCEIVE_FLAGS) -c $< -o $@

# per-kernel VGPR / SGPR / scratch / LDS / occupancy report of the device code (no GPU needed)
resources:
	@mkdir -p $(BUILD)
	$(HIPCC) $(PERCEIVE_FLAGS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c pgtt_perceive.hip -o $(BUILD)/perceive_resources.o

clean:
	rm -rf $(BUILD) $(PERCEIVE_OUT)
