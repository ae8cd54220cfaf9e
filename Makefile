# Build of the MI355X k-mer counting engine (gfx950 only) and its test infrastructure.
#   make            -> yak_amd/libyak_amd.so (HIP kernels + C ABI), yak_amd/libyak_amd_walk.so (the unitig walk on the GPU, a layer
#                      above it), yak_amd/libyak_amd_gfa.so (the links between the unitigs and the GFA, a layer above both),
#                      yak_amd/libyak_amd_path.so (sequences as paths on the unitig graph, a layer above the walk),
#                      yak_amd/libyak_amd_bubble.so (the simple bubbles of the unitig graph, a layer above the gfa),
#                      yak_amd/libyak_amd_clean.so (tips clipped and bubbles popped, a layer above the bubbles),
#                      yak_amd/libyak_amd_correct.so (substitution errors of reads repaired, a layer above libyak_amd.so alone),
#                      yak_amd/libyak_amd_allele.so (the bubbles' alleles supported with reads, a layer above the paths and the bubbles),
#                      yak_amd/libyak_amd_phase.so (those alleles phased from the reads that span two bubbles, a layer above the alleles), yak_amd/yak-amd (CLI),
#                      tools/ (synthetic reads), oracle/ (CPU checker; + oracle/_ref if the
#                      reference sources are present)
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -Wall -Wno-unused-result -Wno-unused-value
CSRC    = yak_amd/csrc
WALK    = yak_amd/walk
GFA     = yak_amd/gfa
PATHD   = yak_amd/path
BUBBLE  = yak_amd/bubble
CLEAN   = yak_amd/clean
CORRECT = yak_amd/correct
ALLELE  = yak_amd/allele
PHASE   = yak_amd/phase

all: lib cli tools oracle

lib: yak_amd/libyak_amd.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_path.so yak_amd/libyak_amd_bubble.so yak_amd/libyak_amd_clean.so yak_amd/libyak_amd_correct.so yak_amd/libyak_amd_allele.so yak_amd/libyak_amd_phase.so
cli: yak_amd/yak-amd

yak_amd/kernels.o: $(CSRC)/kernels.hip $(wildcard $(CSRC)/kern_*.inc) $(CSRC)/yk_device.h $(CSRC)/rec_fmt.h $(CSRC)/replay_plan.h $(CSRC)/count_plan.h $(CSRC)/seg_sort_tile.h $(CSRC)/tally.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/tally.o: $(CSRC)/tally.cpp $(CSRC)/tally.h include/yak_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# every other object of the library: one header list for all of them (a header too many costs a rebuild, one too few a stale object)
ENGDEPS = $(CSRC)/engine_int.h $(CSRC)/dev_buf.h $(CSRC)/tally.h $(CSRC)/engine.h $(CSRC)/table_ranges.h $(CSRC)/yak_file.h $(CSRC)/yk_device.h $(CSRC)/rec_fmt.h $(CSRC)/replay_plan.h $(CSRC)/count_plan.h $(CSRC)/seg_sort_tile.h \
          $(CSRC)/hpc_host.h $(CSRC)/unitig_walk.h $(CSRC)/yak_host.h $(CSRC)/pgz.h $(CSRC)/round_plan.h include/yak.h include/yak_amd.h
yak_amd/%.o: $(CSRC)/%.cpp $(ENGDEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/libyak_amd.so: yak_amd/kernels.o yak_amd/tally.o yak_amd/pool.o yak_amd/engine_ctx.o yak_amd/engine_pass.o yak_amd/engine_acc.o yak_amd/engine_count.o yak_amd/engine_slice.o yak_amd/engine_table.o yak_amd/layout.o yak_amd/table_read.o yak_amd/lookup_dev.o yak_amd/yak_hetmer.o yak_amd/yak_graph.o yak_amd/yak_hpc.o yak_amd/yak_api.o yak_amd/yak_table_ops.o yak_amd/yak_file.o yak_amd/yak_count.o yak_amd/yak_qv_solve.o yak_amd/yak_reader.o yak_amd/yak_multi.o yak_amd/yak_lookup.o yak_amd/yak_inspect.o yak_amd/yak_print.o $(CSRC)/libyak_amd.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -Wl,-Bsymbolic -Wl,--version-script=$(CSRC)/libyak_amd.map -o $@ $(filter %.o,$^) -lz

# The layers above libyak_amd.so (DESIGN.md sections 21 to 24, 26 and 29 to 32): each its own kernels, public calls of the libraries below it only, the shared
# headers of yak_amd/layer/, and tally.o linked in once more: its table is per library behind the version script.
#   $(1) the name and its directory under yak_amd/, $(2) its further headers, $(3) the libraries below it in link order, $(4) further link flags
LAYER     = yak_amd/layer
LAYERDEPS = $(LAYER)/layer_host.h $(LAYER)/layer_dev.h $(LAYER)/layer_seqs.h $(LAYER)/seq_reader.h $(CSRC)/tally.h include/yak.h include/yak_amd.h include/yak_amd_walk.h
define LAYER_LIB
yak_amd/$(1).o: yak_amd/$(1)/$(1).hip $(2) $$(LAYERDEPS)
	$$(HIPCC) $$(HIPFLAGS) -c $$< -o $$@
yak_amd/libyak_amd_$(1).so: yak_amd/$(1).o yak_amd/tally.o $(3) yak_amd/$(1)/libyak_amd_$(1).map
	$$(HIPCC) --offload-arch=$$(ARCH) -shared -Wl,-Bsymbolic -Wl,--version-script=yak_amd/$(1)/libyak_amd_$(1).map -o $$@ $$(filter %.o,$$^) -Lyak_amd \
		$$(patsubst yak_amd/lib%.so,-l%,$$(filter %.so,$$^)) -Wl,-rpath,'$$$$ORIGIN' $(4)
endef
# the device walk of `yak-amd unitigs -g`
$(eval $(call LAYER_LIB,walk,$(WALK)/uwalk_step.h $(WALK)/uwalk_host.h,yak_amd/libyak_amd.so))
# the links between unitigs of `yak-amd unitigs -G`
$(eval $(call LAYER_LIB,gfa,$(GFA)/gfa_step.h $(GFA)/gfa_text.h include/yak_amd_gfa.h,yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so))
# sequences as paths on the unitig graph, `yak-amd paths`; gfa_step.h is a header and makes no link dependency
$(eval $(call LAYER_LIB,path,$(PATHD)/path_step.h $(PATHD)/path_text.h $(GFA)/gfa_step.h include/yak_amd_path.h,yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so,-lz))
# the simple bubbles of the unitig graph, `yak-amd bubbles`; gfa_text.h and gfa_step.h come in as headers for the -s text
$(eval $(call LAYER_LIB,bubble,$(BUBBLE)/bubble_step.h $(BUBBLE)/bubble_text.h $(GFA)/gfa_step.h $(GFA)/gfa_text.h include/yak_amd_gfa.h include/yak_amd_bubble.h,yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so))
# tips clipped and bubbles popped, `yak-amd clean`; the steps and texts of the bubbles and the links come in as headers
$(eval $(call LAYER_LIB,clean,$(CLEAN)/clean_step.h $(CLEAN)/clean_text.h $(BUBBLE)/bubble_step.h $(BUBBLE)/bubble_text.h $(GFA)/gfa_step.h $(GFA)/gfa_text.h include/yak_amd_gfa.h include/yak_amd_bubble.h include/yak_amd_clean.h,yak_amd/libyak_amd_bubble.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so))
# substitution errors of reads repaired, `yak-amd correct`: above libyak_amd.so alone
$(eval $(call LAYER_LIB,correct,$(CORRECT)/correct_step.h $(CORRECT)/correct_text.h include/yak_amd_correct.h,yak_amd/libyak_amd.so,-lz))
# the bubbles' alleles supported with reads, `yak-amd bubbles -r`; the steps and texts of the bubbles and the links come in as headers
$(eval $(call LAYER_LIB,allele,$(ALLELE)/allele_step.h $(ALLELE)/allele_text.h $(BUBBLE)/bubble_step.h $(BUBBLE)/bubble_text.h $(GFA)/gfa_step.h $(GFA)/gfa_text.h include/yak_amd_gfa.h include/yak_amd_path.h include/yak_amd_bubble.h include/yak_amd_allele.h,yak_amd/libyak_amd_path.so yak_amd/libyak_amd_bubble.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so,-lz))
# those alleles phased from the reads that span two bubbles, `yak-amd bubbles -r -p`; the steps and texts of the alleles come in as headers
$(eval $(call LAYER_LIB,phase,$(PHASE)/phase_step.h $(PHASE)/phase_text.h $(ALLELE)/allele_step.h $(ALLELE)/allele_text.h $(BUBBLE)/bubble_step.h $(BUBBLE)/bubble_text.h $(GFA)/gfa_step.h $(GFA)/gfa_text.h include/yak_amd_gfa.h include/yak_amd_path.h include/yak_amd_bubble.h include/yak_amd_allele.h include/yak_amd_phase.h,yak_amd/libyak_amd_allele.so yak_amd/libyak_amd_path.so yak_amd/libyak_amd_bubble.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so,-lz))

yak_amd/yak-amd: $(CSRC)/main.c include/yak.h include/yak_amd.h include/yak_amd_walk.h include/yak_amd_gfa.h include/yak_amd_path.h include/yak_amd_bubble.h include/yak_amd_clean.h include/yak_amd_correct.h include/yak_amd_allele.h include/yak_amd_phase.h yak_amd/libyak_amd.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_path.so yak_amd/libyak_amd_bubble.so yak_amd/libyak_amd_clean.so yak_amd/libyak_amd_correct.so yak_amd/libyak_amd_allele.so yak_amd/libyak_amd_phase.so
	gcc -O2 -Wall -Iinclude $(CSRC)/main.c -o $@ -Lyak_amd -lyak_amd_phase -lyak_amd_allele -lyak_amd_correct -lyak_amd_clean -lyak_amd_bubble -lyak_amd_path -lyak_amd_gfa -lyak_amd_walk -lyak_amd -Wl,-rpath,'$$ORIGIN' -lz

tools:
	$(MAKE) -C tools
oracle: lib
	$(MAKE) -C oracle all ref

clean:
	rm -f yak_amd/*.o yak_amd/libyak_amd.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_path.so yak_amd/libyak_amd_bubble.so yak_amd/libyak_amd_clean.so yak_amd/libyak_amd_correct.so yak_amd/libyak_amd_allele.so yak_amd/libyak_amd_phase.so yak_amd/yak-amd
	$(MAKE) -C tools clean
	$(MAKE) -C oracle clean
.PHONY: all lib cli tools oracle clean
