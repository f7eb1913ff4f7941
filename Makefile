# Top-level build: libbdx.so (HIP, gfx950), the breakdancer-max CLI and the CPU oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := breakdancer_amd/csrc
HOST := breakdancer_amd/host
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result -Iinclude
KERNELS := $(CSRC)/k1_classify.hip $(CSRC)/k2_compact.hip $(CSRC)/k3_regions.hip $(CSRC)/k4_join.hip $(CSRC)/k5_poisson.hip $(CSRC)/k6_assemble.hip $(CSRC)/k7_exchange.hip $(CSRC)/kq_queries.hip $(CSRC)/kp_clip.hip $(CSRC)/kr_depth.hip $(CSRC)/k9_shard.hip $(CSRC)/kz_inflate.hip $(CSRC)/kb_records.hip $(CSRC)/kx_exclude.hip $(CSRC)/kd_markdup.hip $(CSRC)/kc_insert_stats.hip $(CSRC)/kh_insert_hist.hip $(CSRC)/km_mini.hip $(CSRC)/ka_anchor.hip $(CSRC)/bdx_api.hip
OBJS := $(KERNELS:.hip=.o) $(CSRC)/bdx_walk.o $(CSRC)/bdx_walk_reads.o
HOSTCOMMON := $(HOST)/options.cpp $(HOST)/config.cpp $(HOST)/bam_reader.cpp $(HOST)/fast_inflate.cpp $(HOST)/column_reader.cpp $(HOST)/producer.cpp $(HOST)/device_feed.cpp $(HOST)/dumps.cpp $(HOST)/cache.cpp $(HOST)/vcf.cpp $(HOST)/exclude.cpp $(HOST)/sites.cpp $(HOST)/table.cpp $(HOST)/store_counts.cpp $(HOST)/inputs.cpp $(HOST)/estimate.cpp $(HOST)/mini.cpp $(HOST)/anchor.cpp

all: breakdancer_amd/libbdx.so bin/breakdancer-max bin/bdx-dump-reads bin/bam2cfg bin/bdx-inflate-check bin/bdx-sites-check bin/bdx-ci-check bin/bdx-depth-check bin/bdx-mapq-check bin/bdx-clip-check bin/bdx-clip-store bin/bdx-estimate-check bin/bdx-mini-check bin/bdx-anchor-check bin/bdx-table-check bin/bdx-feed-check bin/bdx-feed-probe tests/prims/libbdx_prims.so tests/prims/libbdx_stages.so tests/prims/libbdx_compact.so tests/prims/libbdx_assemble.so oracle

$(CSRC)/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.h) include/bdx.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/bdx_walk.o: $(CSRC)/bdx_walk.cpp $(CSRC)/bdx_walk.h include/bdx.h
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(CSRC)/bdx_walk_reads.o: $(CSRC)/bdx_walk_reads.cpp $(CSRC)/bdx_walk.h $(CSRC)/bdx_dev.h include/bdx.h
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

breakdancer_amd/libbdx.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJS)

HOSTFLAGS := -O2 -std=c++17 -ffp-contract=off -Wall -Iinclude -pthread

bin/breakdancer-max: $(HOSTCOMMON) $(HOST)/main.cpp $(HOST)/phases.cpp $(wildcard $(HOST)/*.h) $(CSRC)/bdx_exclude.h $(CSRC)/bdx_estimate.h $(CSRC)/bdx_mini.h $(CSRC)/bdx_clip.h breakdancer_amd/libbdx.so
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOSTCOMMON) $(HOST)/main.cpp $(HOST)/phases.cpp -Lbreakdancer_amd -lbdx -lz -Wl,-rpath,'$$ORIGIN/../breakdancer_amd' -Wl,-rpath,/opt/rocm/lib

bin/bdx-inflate-check: $(HOST)/inflate_check_main.cpp $(HOST)/fast_inflate.cpp $(HOST)/fast_inflate.h $(HOST)/bgzf.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -O3 -o $@ $(HOST)/inflate_check_main.cpp $(HOST)/fast_inflate.cpp -lz

# test tooling: the --sites parser on its own (tests/test_sites.py builds it a second time under a sanitizer)
bin/bdx-sites-check: $(HOST)/sites_check_main.cpp $(HOST)/sites.cpp $(HOST)/sites.h include/bdx.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/sites_check_main.cpp $(HOST)/sites.cpp

# test tooling: --ci's interval arithmetic (vcf.cpp) on its own (tests/test_ci.py builds it a second time under a sanitizer)
bin/bdx-ci-check: $(HOST)/ci_check_main.cpp $(HOST)/vcf.cpp $(HOST)/vcf.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/ci_check_main.cpp $(HOST)/vcf.cpp

# test tooling: --depth's RDR arithmetic and formatting (vcf.cpp) on its own (tests/test_depth.py)
bin/bdx-depth-check: $(HOST)/depth_check_main.cpp $(HOST)/vcf.cpp $(HOST)/vcf.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/depth_check_main.cpp $(HOST)/vcf.cpp

# test tooling: --mapq's INFO formatting (vcf.cpp) on its own (tests/test_mapq.py)
bin/bdx-mapq-check: $(HOST)/mapq_check_main.cpp $(HOST)/vcf.cpp $(HOST)/vcf.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/mapq_check_main.cpp $(HOST)/vcf.cpp

# test tooling: the host half of --clip -- the clip word (csrc/bdx_clip.h), the host reader's words of a BAM, the INFO keys (vcf.cpp) --
# without libbdx (tests/test_clip.py)
bin/bdx-clip-check: $(HOST)/clip_check_main.cpp $(HOST)/vcf.cpp $(HOST)/vcf.h $(HOST)/bam_reader.cpp $(HOST)/bam_reader.h $(HOST)/bgzf.h $(CSRC)/bdx_clip.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/clip_check_main.cpp $(HOST)/vcf.cpp $(HOST)/bam_reader.cpp -lz

# test tooling: the clip column as a run with --clip leaves it, through the CLI's own feeding phases (tests/test_gpu_clip.py; needs a GPU)
bin/bdx-clip-store: $(HOSTCOMMON) $(HOST)/clip_store_main.cpp $(HOST)/phases.cpp $(wildcard $(HOST)/*.h) $(CSRC)/bdx_exclude.h $(CSRC)/bdx_estimate.h $(CSRC)/bdx_mini.h $(CSRC)/bdx_clip.h breakdancer_amd/libbdx.so
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOSTCOMMON) $(HOST)/clip_store_main.cpp $(HOST)/phases.cpp -Lbreakdancer_amd -lbdx -lz -Wl,-rpath,'$$ORIGIN/../breakdancer_amd' -Wl,-rpath,/opt/rocm/lib

# test tooling: the host half of --estimate (estimate.cpp, csrc/bdx_estimate.h) on a histogram given as text, without libbdx (tests/test_estimate.py)
bin/bdx-estimate-check: $(HOST)/estimate_check_main.cpp $(HOST)/estimate.cpp $(HOST)/config.cpp $(HOST)/estimate.h $(HOST)/config.h $(CSRC)/bdx_estimate.h include/bdx.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/estimate_check_main.cpp $(HOST)/estimate.cpp $(HOST)/config.cpp

# test tooling: the host half of --mini (mini.cpp, csrc/bdx_mini.h) on rows given as text, without libbdx (tests/test_mini.py)
bin/bdx-mini-check: $(HOST)/mini_check_main.cpp $(HOST)/mini.cpp $(HOST)/mini.h $(CSRC)/bdx_mini.h include/bdx.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/mini_check_main.cpp $(HOST)/mini.cpp

# test tooling: the host half of --anchor (anchor.cpp) on rows given as text, without libbdx (tests/test_anchor.py)
bin/bdx-anchor-check: $(HOST)/anchor_check_main.cpp $(HOST)/anchor.cpp $(HOST)/anchor.h $(HOST)/mini.h include/bdx.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/anchor_check_main.cpp $(HOST)/anchor.cpp

# test tooling: the table formatter (table.cpp) on its own, without libbdx (tests/test_table.py builds it again under the sanitizers)
bin/bdx-table-check: $(HOST)/table_check_main.cpp $(HOST)/table.cpp $(HOST)/options.cpp $(HOST)/config.cpp $(HOST)/table.h $(HOST)/options.h $(HOST)/config.h include/bdx.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/table_check_main.cpp $(HOST)/table.cpp $(HOST)/options.cpp $(HOST)/config.cpp

# test tooling: the device feeder's sizing plan, piece cutter and tie rule (feed_plan.h) on their own, without libbdx (tests/test_feed.py
# builds it again under the sanitizers)
bin/bdx-feed-check: $(HOST)/feed_check_main.cpp $(HOST)/feed_plan.h $(HOST)/bgzf.h include/bdx.h
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/feed_check_main.cpp

# test tooling: the shared scan, wave-search, window-walk and insertion-merge headers on their own behind plain C entry points
# (tests/test_gpu_prims.py, tests/test_gpu_insert.py)
tests/prims/libbdx_prims.so: tests/prims/prims.hip $(CSRC)/bdx_scan.h $(CSRC)/bdx_wave_search.h $(CSRC)/bdx_window.h $(CSRC)/bdx_insert.h $(CSRC)/bdx_k3.h $(CSRC)/bdx_dev.h include/bdx.h
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -shared -o $@ $<

# test tooling: the region cut and the mate join on their own -- launch_k3 and launch_k4_join_only with their translation units, unchanged,
# behind plain C entry points (tests/test_gpu_regions.py); nothing of it goes into libbdx.so
tests/prims/libbdx_stages.so: tests/prims/stages.hip $(CSRC)/k3_regions.hip $(CSRC)/k4_join.hip $(CSRC)/bdx_k3.h $(CSRC)/bdx_scan.h $(CSRC)/bdx_dev.h include/bdx.h
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -shared -o $@ tests/prims/stages.hip $(CSRC)/k3_regions.hip $(CSRC)/k4_join.hip

# test tooling: K2 and the pass-1 finalisation on their own -- launch_k2, launch_finalize and launch_k1 with their translation units, unchanged,
# behind plain C entry points (tests/test_gpu_compact.py); nothing of it goes into libbdx.so
tests/prims/libbdx_compact.so: tests/prims/compact.hip $(CSRC)/k1_classify.hip $(CSRC)/k2_compact.hip $(CSRC)/bdx_finalize.h $(CSRC)/bdx_dev.h include/bdx.h
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -shared -Wl,--no-undefined -o $@ tests/prims/compact.hip $(CSRC)/k1_classify.hip $(CSRC)/k2_compact.hip

# test tooling: K6's pair groups, components, device walks and final table on their own -- launch_k6_groups, launch_k6_walk and launch_k6_table with
# their translation unit and the host walk's, unchanged, behind plain C entry points (tests/test_gpu_assemble.py); nothing of it goes into libbdx.so
tests/prims/libbdx_assemble.so: tests/prims/assemble.hip $(CSRC)/k6_assemble.hip $(CSRC)/bdx_walk.cpp $(CSRC)/bdx_walk.h $(CSRC)/bdx_insert.h $(CSRC)/bdx_poisson.h $(CSRC)/bdx_k3.h $(CSRC)/bdx_scan.h $(CSRC)/bdx_dev.h include/bdx.h
	$(HIPCC) $(HIPFLAGS) -I$(CSRC) -shared -Wl,--no-undefined -o $@ tests/prims/assemble.hip $(CSRC)/k6_assemble.hip $(CSRC)/bdx_walk.cpp

# measurement tool (bench.py): the feeder's ceilings -- page cache -> pinned -> HBM
bin/bdx-feed-probe: tools/feed_probe.hip
	@mkdir -p bin
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -mavx2 -o $@ $< -lpthread

bin/bam2cfg: $(HOST)/bam2cfg_main.cpp $(HOST)/bam_reader.cpp $(HOST)/bam_reader.h $(HOST)/bgzf.h $(CSRC)/bdx_clip.h breakdancer_amd/libbdx.so
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOST)/bam2cfg_main.cpp $(HOST)/bam_reader.cpp -Lbreakdancer_amd -lbdx -lz -lpthread -Wl,-rpath,'$$ORIGIN/../breakdancer_amd' -Wl,-rpath,/opt/rocm/lib

bin/bdx-dump-reads: $(HOSTCOMMON) $(HOST)/dump_main.cpp $(wildcard $(HOST)/*.h) $(CSRC)/bdx_exclude.h $(CSRC)/bdx_estimate.h $(CSRC)/bdx_mini.h $(CSRC)/bdx_clip.h breakdancer_amd/libbdx.so
	@mkdir -p bin
	g++ $(HOSTFLAGS) -o $@ $(HOSTCOMMON) $(HOST)/dump_main.cpp -Lbreakdancer_amd -lbdx -lz -Wl,-rpath,'$$ORIGIN/../breakdancer_amd' -Wl,-rpath,/opt/rocm/lib

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(CSRC)/*.o breakdancer_amd/libbdx.so bin/breakdancer-max bin/bdx-dump-reads bin/bam2cfg bin/bdx-feed-probe bin/bdx-inflate-check bin/bdx-sites-check bin/bdx-ci-check bin/bdx-depth-check bin/bdx-mapq-check bin/bdx-clip-check bin/bdx-clip-store bin/bdx-estimate-check bin/bdx-mini-check bin/bdx-anchor-check bin/bdx-table-check bin/bdx-feed-check tests/prims/libbdx_prims.so tests/prims/libbdx_stages.so tests/prims/libbdx_compact.so tests/prims/libbdx_assemble.so
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
