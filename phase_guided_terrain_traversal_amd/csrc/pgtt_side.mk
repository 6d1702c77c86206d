# The side libraries, libpgtt_<name>.so (include/pgtt_<name>.h): hand-written HIP for gfx950, one translation unit pgtt_<name>.hip each.
#   make -f pgtt_side.mk -j8
# Libraries of their own: csrc/Makefile, libpgtt.so and the source hash pgtt_build_info() embeds are not touched by this file.
# What a unit is built from is stated once, in ../srchash.py (SIDE_SOURCES): this file asks it for the unit's prerequisites (--files) and for
# the hash pgtt_<name>_build_info() reports ("src=<srchash.side_sha256(name)>;flavor=...").
# An experiment build names the libraries it is about and goes elsewhere (it is not shipped); EXTRA reaches those libraries only.
# The depth camera with the per-env cull switched off (flavor "nocull"; DESIGN.md 14 quotes its time):
#   make -f pgtt_side.mk LIBS=depth EXTRA=-DPGTT_DEPTH_NOCULL BUILD=build/depth_nocull OUTDIR=build/depth_nocull SUFFIX=_nocull
# A build that names its own flavor:
#   make -f pgtt_side.mk LIBS=learn EXTRA='-DPGTT_LEARN_FLAVOR=\"trial\"' BUILD=build/learn_trial OUTDIR=build/learn_trial SUFFIX=_trial
HIPCC ?= hipcc
ARCH ?= gfx950
PYTHON ?= python3
LIBS ?= render depth perceive elevation learn lidar
BUILD ?= build/side
OUTDIR ?= ..
SUFFIX ?=
EXTRA ?=
FLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value
# in a recipe of the unit $*: -DPGTT_<NAME>_SRC=\"<hash>\"
DEFS = -DPGTT_$(shell echo $* | tr a-z A-Z)_SRC=\"$(HASH_$*)\" $(EXTRA)
OUTS = $(foreach l,$(LIBS),$(OUTDIR)/libpgtt_$(l)$(SUFFIX).so)
OBJS = $(foreach l,$(LIBS),$(BUILD)/$(l).o)

define ask_srchash
FILES_$(1) := $$(shell $$(PYTHON) ../srchash.py --files $(1))
HASH_$(1) := $$(shell $$(PYTHON) ../srchash.py $(1))
ifeq ($$(and $$(FILES_$(1)),$$(HASH_$(1))),)
$$(error ../srchash.py printed no files or no hash for "$(1)" (is $$(PYTHON) on PATH?): the library would not say what it was built from)
endif
endef
$(foreach l,$(LIBS),$(eval $(call ask_srchash,$(l))))

all: $(OUTS)

.PHONY: all clean resources asm FORCE
# the objects stay: a second run recompiles nothing
.SECONDARY: $(OBJS)
.SECONDEXPANSION:

$(OUTDIR)/libpgtt_%$(SUFFIX).so: $(BUILD)/%.o
	@mkdir -p $(OUTDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(BUILD)/%.o: pgtt_%.hip $$(FILES_$$*)
	@mkdir -p $(BUILD)
	$(HIPCC) $(FLAGS) $(DEFS) -c $< -o $@

# per-kernel VGPR / SGPR / scratch / LDS / occupancy report of the device code of $(LIBS) (no GPU needed)
resources: $(foreach l,$(LIBS),$(BUILD)/$(l)_resources.o)

$(BUILD)/%_resources.o: pgtt_%.hip FORCE
	@mkdir -p $(BUILD)
	$(HIPCC) $(FLAGS) $(DEFS) --cuda-device-only -Rpass-analysis=kernel-resource-usage -c $< -o $@

# the device assembly of $(LIBS), $(BUILD)/<lib>.s: what tools/side_isa_diff.py compares between two trees (no GPU needed)
asm: $(foreach l,$(LIBS),$(BUILD)/$(l).s)

$(BUILD)/%.s: pgtt_%.hip FORCE
	@mkdir -p $(BUILD)
	$(HIPCC) $(FLAGS) $(DEFS) --cuda-device-only -S $< -o $@

FORCE:

clean:
	rm -rf $(BUILD) $(OUTS)
