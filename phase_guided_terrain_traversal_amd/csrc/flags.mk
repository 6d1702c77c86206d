# flags.mk - the compiler flags of the physics_kernel translation units (included by the Makefile).  With the sources of pgtt_physics_inst.hip
# this text, comments apart, is what the library's source hash covers (../srchash.py): an edit here rebuilds every physics object and gives the
# library a new pgtt_build_info().  ARCH, DIVFLAG (PRECISE_DIV) and EXTRA come from the Makefile; a build that changes them says so in its flavor.
# -fno-slp-vectorize: the SLP vectoriser pairs the scalar fp32 chains into v_pk_* ops at the price of register-pair
# shuffles and scratch spills; without it the flat kernels need no scratch and run 8-17 % faster (profiles/archive/r01d_*).
# fp32 `/` and sqrtf() are CORRECTLY ROUNDED in the product (hipcc's default; what XLA emits for the reference's jnp arithmetic).  The step has
# ~380 divisions and ~60 square roots per substep (Cholesky, back-substitution, line search, impedances); the 1-ulp forms
# (-fno-hip-fp32-correctly-rounded-divide-sqrt: v_rcp / v_sqrt plus one refinement instead of the 11- / 17-instruction sequences) were the product
# until round 4 and bought 0 - 4 % (driver record r04: 22.15 M with them, 22.36 M without) - not worth a precision footnote.  `make fastdiv` still
# builds them as ../libpgtt_fastdiv.so (two kernel variants only) so that bench.py keeps the price of correct rounding driver-visible.
# -mllvm -amdgpu-sched-strategy=iterative-ilp: the step runs ONE wave per SIMD, so nothing but instruction-level parallelism
# hides VALU / LDS latency; the ILP-driven iterative scheduler gives 4-5 % over the default (max-occupancy) one
# (level4 12.9 -> 13.4 M, flat 20.4 -> 21.5 M env-steps/s; max-ilp, iterative-minreg and max-memory-clause measured no better).
BASEFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wno-unused-value -fno-slp-vectorize $(DIVFLAG) $(EXTRA)
# -mllvm -amdgpu-load-store-vectorizer=0: the IR-level merging of neighbouring loads / stores (the model-constant and per-env-model reads of
# the prologue and the kinematics stage) lengthens live ranges in a kernel that sits at 256 VGPRs + ~247 AGPRs; without it the terrain step
# kernels are 0.6 - 0.8 % faster (hex 4096 envs 169.1 -> 168.1 us, oct 8192 envs WFC + DR 254.8 -> 252.7 us, flat unchanged), bit-identical
# on every workload of tools/gpu_ab_bitwise.py incl. the oct layout.  The rest of a sweep of 18 scheduler / LICM / sink / if-conversion /
# -O2 / -Os settings measured 0.7 - 4 % SLOWER (docs/HISTORY.md 5.6).
FLAGS = $(BASEFLAGS) -mllvm -amdgpu-sched-strategy=iterative-ilp -mllvm -amdgpu-load-store-vectorizer=0
# per-variant additions.  oct + DR + box terrain (configs[3]'s kernel) is the one variant that spilled under correct rounding (12 B per lane, reloaded inside
# the line-search rounds): with the register allocator splitting live ranges for size instead of speed it fits (0 B), 249.4 -> 243.6 us at 8192 envs, bit-identical
# (profiles/r05_oct_dr_alloc.txt).  The same switch on the hex kernels was measured in round 3 and did not survive (docs/HISTORY.md 5.6).
FLAGS_2_0_1_1 = -mllvm -split-spill-mode=size
FLAGS_2_2_1_1 = -mllvm -split-spill-mode=size
# compiler flags of physics variant $(1) (SUBS_MODE_DR_TERRAIN): what its object, `make resources` and `make flags-<variant>` use
vflags = $(FLAGS) $(FLAGS_$(1)) -DPG_SUBS=$(word 1,$(subst _, ,$(1))) -DPG_MODE=$(word 2,$(subst _, ,$(1))) -DPG_DR=$(word 3,$(subst _, ,$(1))) -DPG_TERRAIN=$(word 4,$(subst _, ,$(1)))
