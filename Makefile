# Build of the MI355X k-mer counting engine (gfx950 only) and its test infrastructure.
#   make            -> yak_amd/libyak_amd.so (HIP kernels + C ABI), yak_amd/libyak_amd_walk.so (the unitig walk on the GPU, a layer
#                      above it), yak_amd/libyak_amd_gfa.so (the links between the unitigs and the GFA, a layer above both),
#                      yak_amd/libyak_amd_path.so (sequences as paths on the unitig graph, a layer above the walk), yak_amd/yak-amd (CLI),
#                      tools/ (synthetic reads), oracle/ (CPU checker; + oracle/_ref if the
#                      reference sources are present)
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -Wall -Wno-unused-result -Wno-unused-value
CSRC    = yak_amd/csrc
WALK    = yak_amd/walk
GFA     = yak_amd/gfa
PATHD   = yak_amd/path

all: lib cli tools oracle

lib: yak_amd/libyak_amd.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_path.so
cli: yak_amd/yak-amd

yak_amd/kernels.o: $(CSRC)/kernels.hip $(wildcard $(CSRC)/kern_*.inc) $(CSRC)/yk_device.h $(CSRC)/replay_plan.h $(CSRC)/seg_sort_tile.h $(CSRC)/tally.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/tally.o: $(CSRC)/tally.cpp $(CSRC)/tally.h include/yak_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# every other object of the library: one header list for all of them (a header too many costs a rebuild, one too few a stale object)
ENGDEPS = $(CSRC)/engine_int.h $(CSRC)/dev_buf.h $(CSRC)/tally.h $(CSRC)/engine.h $(CSRC)/table_ranges.h $(CSRC)/yk_device.h $(CSRC)/replay_plan.h $(CSRC)/seg_sort_tile.h \
          $(CSRC)/hpc_host.h $(CSRC)/unitig_walk.h $(CSRC)/yak_host.h $(CSRC)/pgz.h $(CSRC)/round_plan.h include/yak.h include/yak_amd.h
yak_amd/%.o: $(CSRC)/%.cpp $(ENGDEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/libyak_amd.so: yak_amd/kernels.o yak_amd/tally.o yak_amd/pool.o yak_amd/engine_ctx.o yak_amd/engine_pass.o yak_amd/engine_slice.o yak_amd/engine_table.o yak_amd/layout.o yak_amd/table_read.o yak_amd/lookup_dev.o yak_amd/yak_hetmer.o yak_amd/yak_graph.o yak_amd/yak_hpc.o yak_amd/yak_api.o yak_amd/yak_count.o yak_amd/yak_qv_solve.o yak_amd/yak_reader.o yak_amd/yak_multi.o yak_amd/yak_lookup.o yak_amd/yak_inspect.o yak_amd/yak_print.o $(CSRC)/libyak_amd.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -Wl,-Bsymbolic -Wl,--version-script=$(CSRC)/libyak_amd.map -o $@ $(filter %.o,$^) -lz

# the device walk of `yak-amd unitigs -g`: its own kernels and its own launch tally (tally.cpp a second time), public calls
# of libyak_amd.so only
yak_amd/walk.o: $(WALK)/walk.hip $(WALK)/uwalk_step.h $(WALK)/uwalk_host.h $(CSRC)/tally.h include/yak.h include/yak_amd.h include/yak_amd_walk.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/walk_tally.o: $(CSRC)/tally.cpp $(CSRC)/tally.h include/yak_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/libyak_amd_walk.so: yak_amd/walk.o yak_amd/walk_tally.o yak_amd/libyak_amd.so $(WALK)/libyak_amd_walk.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -Wl,-Bsymbolic -Wl,--version-script=$(WALK)/libyak_amd_walk.map -o $@ $(filter %.o,$^) -Lyak_amd -lyak_amd -Wl,-rpath,'$$ORIGIN'

# the links between unitigs of `yak-amd unitigs -G`: its own kernels and its own launch tally (tally.cpp a third time),
# public calls of the two libraries below it only
yak_amd/gfa.o: $(GFA)/gfa.hip $(GFA)/gfa_step.h $(GFA)/gfa_text.h $(CSRC)/tally.h include/yak.h include/yak_amd.h include/yak_amd_walk.h include/yak_amd_gfa.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/gfa_tally.o: $(CSRC)/tally.cpp $(CSRC)/tally.h include/yak_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/libyak_amd_gfa.so: yak_amd/gfa.o yak_amd/gfa_tally.o yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so $(GFA)/libyak_amd_gfa.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -Wl,-Bsymbolic -Wl,--version-script=$(GFA)/libyak_amd_gfa.map -o $@ $(filter %.o,$^) -Lyak_amd -lyak_amd_walk -lyak_amd -Wl,-rpath,'$$ORIGIN'

# sequences as paths on the unitig graph, `yak-amd paths`: its own kernels and its own launch tally (tally.cpp a fourth
# time), public calls of the walk's library and of libyak_amd.so only; gfa_step.h is a header and makes no link dependency
yak_amd/path.o: $(PATHD)/path.hip $(PATHD)/path_step.h $(PATHD)/path_text.h $(PATHD)/path_reader.h $(GFA)/gfa_step.h $(CSRC)/tally.h include/yak.h include/yak_amd.h include/yak_amd_walk.h include/yak_amd_path.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/path_tally.o: $(CSRC)/tally.cpp $(CSRC)/tally.h include/yak_amd.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
yak_amd/libyak_amd_path.so: yak_amd/path.o yak_amd/path_tally.o yak_amd/libyak_amd_walk.so yak_amd/libyak_amd.so $(PATHD)/libyak_amd_path.map
	$(HIPCC) --offload-arch=$(ARCH) -shared -Wl,-Bsymbolic -Wl,--version-script=$(PATHD)/libyak_amd_path.map -o $@ $(filter %.o,$^) -Lyak_amd -lyak_amd_walk -lyak_amd -Wl,-rpath,'$$ORIGIN' -lz

yak_amd/yak-amd: $(CSRC)/main.c include/yak.h include/yak_amd.h include/yak_amd_walk.h include/yak_amd_gfa.h include/yak_amd_path.h yak_amd/libyak_amd.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_path.so
	gcc -O2 -Wall -Iinclude $(CSRC)/main.c -o $@ -Lyak_amd -lyak_amd_path -lyak_amd_gfa -lyak_amd_walk -lyak_amd -Wl,-rpath,'$$ORIGIN' -lz

tools:
	$(MAKE) -C tools
oracle: lib
	$(MAKE) -C oracle all ref

clean:
	rm -f yak_amd/*.o yak_amd/libyak_amd.so yak_amd/libyak_amd_walk.so yak_amd/libyak_amd_gfa.so yak_amd/libyak_amd_path.so yak_amd/yak-amd
	$(MAKE) -C tools clean
	$(MAKE) -C oracle clean
.PHONY: all lib cli tools oracle clean
