# libpgtt_learn.so (include/pgtt_learn.h): the native PPO minibatch update's kernels next to pgtt_ppo.hip, hand-written HIP for gfx950, one translation unit.
#   make -f pgtt_learn.mk
# A library of its own: csrc/Makefile, libpgtt.so, the other side libraries and the source hashes they embed are not touched by this file.
# An experiment build names its flavor and goes elsewhere (it is not shipped):
#   make -f pgtt_learn.mk EXTRA='-DPGTT_LEARN_FLAVOR=\"trial\"' BUILD=build/learn_trial LEARN_OUT=build/learn_trial/libpgtt_learn_trial.so build/learn_trial/libpgtt_learn_trial.so
HIPCC ?= hipcc
ARCH ?= gfx950
BUILD ?= build/learn
EXTRA ?=
LEARN_OUT ?= ../libpgtt_learn.so
LEARN_HDR = ../../include/pgtt_learn.h ../../include/pgtt.h
# pgtt_learn_build_info(): "src=<srchash.side_sha256("learn"): the unit's include closure, comments and white space removed>;flavor=..."
LEARN_FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value -DPGTT_LEARN_SRC=\"$(shell python3 ../srchash.py learn)\" $(EXTRA)

all: $(LEARN_OUT)

.PHONY: all clean resources

$(LEARN_OUT): $(BUILD)/learn.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(BUILD)/learn.o: pgtt_learn.hip $(LEARN_HDR)
	@mkdir -p $(BUILD)
	$(HIPCC) $(LEARN_FLAGS) -c $< -o $@

# per-kernel VGPR / SGPR / scratch / LDS / occupancy report of the device code (no GPU needed)
resources:
	@mkdir -p $(BUILD)
	$(HIPCC) $(LEARN_FLAGS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c pgtt_learn.hip -o $(BUILD)/learn_resources.o

clean:
	rm -rf $(BUILD) $(LEARN_OUT)
