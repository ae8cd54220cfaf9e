/*
 * main.c -- `yak-amd`: the repo's own small command-line driver of libyak_amd.so, plain C against
 * include/yak.h (and include/yak_amd.h for triobin and -X).  It is a test and benchmark vehicle (tests/, bench.py's e2e_cli figure), not a
 * re-creation of the reference's CLI: that one runs unmodified on the library (INTEGRATION.md section 2,
 * oracle/_ref/yak_on_amd).  Thirteen sub-commands -- the reference's whole list -- drive the call sequences the library serves:
 *     count    the counting protocol behind reference main.c:53-61 (one pass, or two passes + shrink
 *              when a bloom filter is asked for)
 *     qv       the lookup protocol behind reference main.c:163-215 (restore, histogram, yak_qv, solve)
 *     triobin  the read binning of reference triobin.c:153-197 (two TRIOBIN loads, yakamd_triobin)
 *     trioeval the phasing evaluation of reference trioeval.c:153-212 (two TRIOBIN loads, yakamd_trioeval)
 *     inspect  the table statistics of reference inspect.c (yakamd_inspect: the k-mer histogram of one table, or the joint
 *              spectrum of two; -R probes the second table as inspect.c:58 does)
 *     chkerr   the streaks of low k-mers of reference chkerr.c:99-133 (yak_ch_restore, yakamd_chkerr)
 *     sexchr   the sex-chromosome tally of reference sexchr.c:104-140 (three SEXCHR loads, yakamd_sexchr)
 *     print    the k-mers of a table as text, reference main.c:286-323 (restore, tighten, yakamd_print)
 *     cntasm   the per-assembly presence counts of reference main.c:90-161 (yak_count per file, shrink / setcnt / merge, tighten)
 *     recount  the counts of a table's k-mers in other sequences, reference main.c:66-88 (restore, tighten, yak_recount)
 *     subtract, isec   the k-mers of the first table absent from / present in the others, reference main.c:217-284
 *     version  the library's YAKS_VERSION
 * and nine beyond the reference: sum (yakamd_ch_sum), depth (yakamd_depth: the depth of every sequence or window in a count table), hetmers
 * (yakamd_hetmers: the pairs of k-mers of a count table that differ in the middle base alone), cover (yakamd_cover: the bases of every sequence
 * that lie inside k-mers a table holds, lacks or holds too often -- as a table, as intervals or as a masked FASTA), unitigs (yakamd_unitigs: the
 * de Bruijn graph the k-mers of a count table span, as its unitigs in FASTA or as its tallies), paths (yakamd_paths: the sequences of a file as
 * paths through those unitigs, as GAF or as tallies per sequence), bubbles (yakamd_bubbles: the forks of that graph whose two arms join again,
 * with their types and alleles; with -r yakamd_alleles: the reads of a file that pass each allele, a call per bubble and the alleles per read), clean (yakamd_clean: the table without the k-mers of that graph's tips and weaker bubble arms) and correct
 * (yakamd_correct: reads with their single substitution errors repaired against a table).  `count -c` and `qv -c` work in homopolymer-compressed
 * space (yakamd_count_hpc; yakamd_ch_set_hpc on the restored table): every run of one base is one base before k-mers are taken.
 * Option letters follow the reference so that test command lines can be shared; the parser, the
 * sub-command table and the usage texts are this file's own.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "yak.h"
#include "yak_amd_walk.h"  /* yakamd_unitigs_dev (unitigs -g) */
#include "yak_amd_gfa.h"   /* yakamd_unitigs_gfa (unitigs -G) */
#include "yak_amd_path.h"  /* yakamd_paths (paths) */
#include "yak_amd_bubble.h" /* yakamd_bubbles (bubbles) */
#include "yak_amd_allele.h" /* yakamd_alleles (bubbles -r) */
#include "yak_amd_phase.h" /* yakamd_phase (bubbles -r -p) */
#include "yak_amd_clean.h" /* yakamd_clean (clean) */
#include "yak_amd_correct.h" /* yakamd_correct (correct) */
#include "yak_amd.h"       /* beyond yak.h: yakamd_test_set (-X), yakamd_triobin, yakamd_trioeval, yakamd_inspect, yakamd_chkerr, yakamd_sexchr, yakamd_print, yakamd_ch_sum, yakamd_depth, yakamd_hetmers, yakamd_cover, yakamd_unitigs, yakamd_count_hpc and yakamd_ch_set_hpc */

/* ---- a table-driven option scanner: "-x", "-xVALUE" and "-x VALUE"; stops at the first non-option ---- */
enum arg_kind { ARG_FLAG, ARG_I32, ARG_SIZE, ARG_I64SIZE, ARG_F64, ARG_TEXT };
struct arg_def { char letter; enum arg_kind kind; void *dst; const char *what; };

static double with_suffix(const char *s)                     /* 64m, 3.2g, 100k: decimal multipliers */
{
	char *end = 0;
	double v = strtod(s, &end);
	switch (end ? *end : 0) {
	case 'k': case 'K': return v * 1e3;
	case 'm': case 'M': return v * 1e6;
	case 'g': case 'G': return v * 1e9;
	default: return v;
	}
}

static void arg_store(const struct arg_def *d, const char *text)
{
	switch (d->kind) {
	case ARG_FLAG: *(int*)d->dst = 1; break;
	case ARG_I32: *(int32_t*)d->dst = (int32_t)strtol(text, 0, 10); break;
	case ARG_SIZE: *(int32_t*)d->dst = (int32_t)(with_suffix(text) + .499); break;
	case ARG_I64SIZE: *(int64_t*)d->dst = (int64_t)(with_suffix(text) + .499); break;
	case ARG_F64: *(double*)d->dst = strtod(text, 0); break;
	case ARG_TEXT: *(const char**)d->dst = text; break;
	}
}

/* returns the index of the first positional argument, or -1 after reporting a bad option */
static int arg_scan(int argc, char **argv, const struct arg_def *defs, int n_defs)
{
	int i = 1;
	for (; i < argc; ++i) {
		const char *a = argv[i];
		if (a[0] != '-' || a[1] == 0) break;
		if (a[1] == '-' && a[2] == 0) { ++i; break; }
		for (const char *q = a + 1; *q; ++q) {               /* flags may be grouped; a valued option ends the group */
			const struct arg_def *d = 0;
			for (int j = 0; j < n_defs; ++j) if (defs[j].letter == *q) d = &defs[j];
			if (!d) { fprintf(stderr, "yak-amd: unknown option -%c\n", *q); return -1; }
			if (d->kind == ARG_FLAG) { arg_store(d, 0); continue; }
			if (q[1]) arg_store(d, q + 1);
			else if (i + 1 < argc) arg_store(d, argv[++i]);
			else { fprintf(stderr, "yak-amd: option -%c needs a value\n", *q); return -1; }
			break;
		}
	}
	return i;
}

static void arg_help(const char *synopsis, const struct arg_def *defs, int n_defs)
{
	fprintf(stderr, "usage: yak-amd %s\n", synopsis);
	for (int j = 0; j < n_defs; ++j) fprintf(stderr, "    -%c%s  %s\n", defs[j].letter, defs[j].kind == ARG_FLAG ? "     " : " VAL ", defs[j].what);
}

/* ---- the table of a command ---- */
/* k and pre of a .yak file's header (htab.c:381-384); 0 if it cannot be read */
static int yak_header(const char *fn, uint32_t *k, uint32_t *pre)
{
	int k_ = 0, pre_ = 0;
	if (yakamd_yak_header(fn, &k_, &pre_) != 0) return 0;
	*k = (uint32_t)k_; *pre = (uint32_t)pre_;
	return 1;
}

/* why a command takes no table of an even k, or of a k from 32 on */
#define K_ODD_GRAPH "the graph is defined for an odd k only"
#define K_ODD_MIDDLE "a k-mer of even length has no middle base"
#define K_32_LOOKUP "the per-position lookup serves k below 32 only"
#define K_32_GRAPH "k must be below 32"
#define K_32_HASH "a k-mer can be rebuilt from its hash for k below 32 only"

/* the k of the table in fn, read from its header before anything is loaded; -1 after the message if the file is no .yak file, if k is even and
 * `odd_why` says why that will not do, or if k is 32 or more and `why_32` says the same: the caller returns 2 */
static int table_k(const char *cmd, const char *fn, const char *odd_why, const char *why_32)
{
	uint32_t k = 0, pre = 0;
	if (!yak_header(fn, &k, &pre)) { fprintf(stderr, "yak-amd %s: %s is not a readable .yak file\n", cmd, fn); return -1; }
	if (odd_why && !(k & 1)) { fprintf(stderr, "yak-amd %s: %s has k = %u: %s\n", cmd, fn, k, odd_why); return -1; }
	if (why_32 && k >= 32) { fprintf(stderr, "yak-amd %s: %s has k = %u: %s\n", cmd, fn, k, why_32); return -1; }
	return (int)k;
}

/* -c of the commands that take a k-mer below it for absent or weak; 0 after the message: the caller returns 1 */
static int min_cnt_ok(const char *cmd, int min_cnt)
{
	if (min_cnt >= 1 && min_cnt <= 1023) return 1;
	fprintf(stderr, "yak-amd %s: -c must be in [1, 1023]\n", cmd);
	return 0;
}

/* the table of fn on the device; 0 after the message: the caller returns 2 */
static yak_ch_t *table_load(const char *cmd, const char *fn)
{
	yak_ch_t *tab = yak_ch_restore(fn);
	if (!tab) fprintf(stderr, "yak-amd %s: cannot load %s (or no MI355X)\n", cmd, fn);
	return tab;
}

/* ---- count ---- */
static int cmd_count(int argc, char **argv)
{
	yak_copt_t o;
	const char *out = 0;
	int hpc = 0;
	yak_copt_init(&o);
	const struct arg_def defs[] = {
		{ 'k', ARG_I32, &o.k, "k-mer length, below 64 (counts are approximate from 32 on)" },
		{ 'p', ARG_I32, &o.pre, "bits of the hash that pick the sub-table" },
		{ 'b', ARG_I32, &o.bf_shift, "log2 bits of the bloom prefilter; 0 = one pass, singletons kept" },
		{ 'H', ARG_SIZE, &o.bf_n_hash, "probes per bloom lookup" },
		{ 't', ARG_I32, &o.n_thread, "host threads (parser)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per host batch" },
		{ 'o', ARG_TEXT, &out, "write the table (.yak) here" },
		{ 'c', ARG_FLAG, &hpc, "count in homopolymer-compressed space: every run of one base is one base (compacted on the device)" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first >= argc) { arg_help("count [options] <reads.fa|fq[.gz]> [second-pass reads]", defs, nd); return 1; }
	if (o.pre < YAK_COUNTER_BITS || o.k < 1 || o.k >= 64) { fprintf(stderr, "yak-amd count: need 1 <= k < 64 and p >= %d\n", YAK_COUNTER_BITS); return 1; }
	if (o.k >= 32) fprintf(stderr, "yak-amd count: k >= 32 uses the 64-bit sum hash: counts are approximate\n");
	const char *pass1 = argv[first], *pass2 = first + 1 < argc ? argv[first + 1] : argv[first];
	yak_ch_t *tab = hpc ? yakamd_count_hpc(pass1, &o, 0) : yak_count(pass1, &o, 0);
	if (!tab) { fprintf(stderr, "yak-amd count: no table (unreadable input, or no MI355X)\n"); return 2; }
	if (o.bf_shift > 0) {                                    /* filtered mode: pass 1 picked the keys, pass 2 counts them */
		yak_ch_destroy_bf(tab);
		yak_ch_clear(tab, o.n_thread);
		if (!(hpc ? yakamd_count_hpc(pass2, &o, tab) : yak_count(pass2, &o, tab))) { yak_ch_destroy(tab); return 2; }
		yak_ch_shrink(tab, 2, YAK_MAX_COUNT, o.n_thread);
		fprintf(stderr, "[M::yak-amd] %ld distinct k-mers after shrinking\n", (long)tab->tot);
	}
	int rc = 0;
	if (out && yak_ch_dump(tab, out) != 0) { fprintf(stderr, "yak-amd count: cannot write %s\n", out); rc = 3; }
	yak_ch_destroy(tab);
	return rc;
}

/* ---- qv ---- */
static const char *const qv_legend[] = {                     /* output format of `yak qv` (reference main.c:196-201) */
	"CC\tCT  kmer_occurrence    short_read_kmer_count  raw_input_kmer_count  adjusted_input_kmer_count",
	"CC\tFR  fpr_lower_bound    fpr_upper_bound",
	"CC\tER  total_input_kmers  adjusted_error_kmers",
	"CC\tCV  coverage",
	"CC\tQV  raw_quality_value  adjusted_quality_value",
	"CC",
};

static int cmd_qv(int argc, char **argv)
{
	yak_qopt_t o;
	int hpc = 0;
	yak_qopt_init(&o);
	const struct arg_def defs[] = {
		{ 'l', ARG_SIZE, &o.min_len, "skip sequences shorter than this" },
		{ 'f', ARG_F64, &o.min_frac, "skip sequences with a smaller share of known k-mers" },
		{ 'e', ARG_F64, &o.fpr, "assumed false-positive rate of \"absent\"" },
		{ 'p', ARG_FLAG, &o.print_each, "one SQ line per sequence" },
		{ 'E', ARG_FLAG, &o.print_err_kmer, "one EK line per absent k-mer run" },
		{ 't', ARG_I32, &o.n_threads, "host threads" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per device batch" },
		{ 'c', ARG_FLAG, &hpc, "the table was counted with `count -c`: compress the sequences too (lengths and positions are then compressed ones)" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("qv [options] <table.yak> <sequences.fa>", defs, nd); return 1; }
	yak_ch_t *tab = table_load("qv", argv[first]);
	if (!tab) return 2;
	if (hpc && yakamd_ch_set_hpc(tab, 1) != 0) { yak_ch_destroy(tab); return 2; }
	static int64_t in_table[YAK_N_COUNTS], in_seqs[YAK_N_COUNTS];
	static yak_qstat_t st;
	const int k = tab->k;
	yak_ch_hist(tab, in_table, o.n_threads);
	for (size_t i = 0; i < sizeof(qv_legend) / sizeof(qv_legend[0]); ++i) puts(qv_legend[i]);
	yak_qv(&o, argv[first + 1], tab, in_seqs);
	yak_qv_solve(in_table, in_seqs, k, o.fpr, &st);
	for (int c = YAK_N_COUNTS; c-- > 0;) printf("CT\t%d\t%ld\t%ld\t%.3f\n", c, (long)in_table[c], (long)in_seqs[c], st.adj_cnt[c]);
	printf("FR\t%.3g\t%.3g\n", st.fpr_lower, st.fpr_upper);
	printf("ER\t%ld\t%.3f\n", (long)st.tot, st.err);
	printf("CV\t%.3f\n", st.cov);
	printf("QV\t%.3f\t%.3f\n", st.qv_raw, st.qv);
	yak_ch_destroy(tab);
	return 0;
}

/* ---- triobin, trioeval ---- */
/* both parents' classes in one table (reference triobin.c:187-188), from argv[first] and argv[first + 1]; 0 after a message */
static yak_ch_t *load_trio(char **argv, int first, int min_cnt, int mid_cnt, const char *cmd)
{
	yak_ch_t *tab = yak_ch_restore_core(0, argv[first], YAK_LOAD_TRIOBIN1, min_cnt, mid_cnt);
	if (tab) tab = yak_ch_restore_core(tab, argv[first + 1], YAK_LOAD_TRIOBIN2, min_cnt, mid_cnt);
	if (!tab) fprintf(stderr, "yak-amd %s: cannot load %s and %s (or no MI355X)\n", cmd, argv[first], argv[first + 1]);
	return tab;
}

static int cmd_triobin(int argc, char **argv)
{
	yakamd_tbopt_t o;
	int min_cnt = 2, mid_cnt = 5;                            /* reference triobin.c:156 */
	yakamd_tbopt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &min_cnt, "min occurrence in a parent" },
		{ 'd', ARG_I32, &mid_cnt, "mid occurrence in a parent (solid)" },
		{ 'r', ARG_F64, &o.ratio_thres, "ratio threshold" },
		{ 't', ARG_I32, &o.n_threads, "host threads (accepted for the reference's command line)" },
		{ 'p', ARG_FLAG, &o.print_diff, "print the positions where the parents differ (D lines)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per chunk" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 2 >= argc) { arg_help("triobin [options] <pat.yak> <mat.yak> <seq.fa>", defs, nd); return 1; }
	yak_ch_t *tab = load_trio(argv, first, min_cnt, mid_cnt, "triobin");
	if (!tab) return 2;
	const int rc = yakamd_triobin(&o, tab, argv[first + 2], 0) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

static int cmd_trioeval(int argc, char **argv)
{
	yakamd_teopt_t o;
	int min_cnt = 2, mid_cnt = 5, no_frag = 0;               /* reference trioeval.c:158 */
	yakamd_teopt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &min_cnt, "min occurrence in a parent" },
		{ 'd', ARG_I32, &mid_cnt, "mid occurrence in a parent (solid)" },
		{ 'n', ARG_I32, &o.min_n, "min streak" },
		{ 't', ARG_I32, &o.n_threads, "host threads (accepted for the reference's command line)" },
		{ 'e', ARG_FLAG, &o.print_err, "print the switch positions (E lines)" },
		{ 'F', ARG_FLAG, &no_frag, "do not print the fragments (F lines)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per chunk" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 2 >= argc) { arg_help("trioeval [options] <pat.yak> <mat.yak> <seq.fa>", defs, nd); return 1; }
	if (no_frag) o.print_frag = 0;
	yak_ch_t *tab = load_trio(argv, first, min_cnt, mid_cnt, "trioeval");
	if (!tab) return 2;
	static int64_t cnt[YAK_N_COUNTS];
	yak_ch_hist(tab, cnt, o.n_threads);
	fprintf(stderr, "[M::%s] %ld file1-specific k-mers and %ld file2-specific k-mers\n", "main_trioeval", (long)cnt[0<<2|2], (long)cnt[2<<2|0]);
	const int rc = yakamd_trioeval(&o, tab, argv[first + 2], 0) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- inspect ---- */
static int cmd_inspect(int argc, char **argv)
{
	yakamd_inopt_t o;
	yakamd_inopt_init(&o);
	const struct arg_def defs[] = {
		{ 'm', ARG_I32, &o.max_cnt, "max count (effective with in2.yak)" },
		{ 'R', ARG_FLAG, &o.ref_probe, "probe in2.yak with the stored key, as the reference's inspect.c:58 does" },
		{ 't', ARG_I32, &o.n_threads, "host threads" },
		{ 'B', ARG_I64SIZE, &o.batch_keys, "keys of in1.yak per device batch" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first >= argc || argc - first > 2) { arg_help("inspect [options] <in1.yak> [in2.yak]", defs, nd); return 1; }
	return yakamd_inspect(&o, argv[first], first + 1 < argc ? argv[first + 1] : 0, 0) == 0 ? 0 : 2;
}

/* ---- chkerr ---- */
static int cmd_chkerr(int argc, char **argv)
{
	yakamd_ceopt_t o;
	yakamd_ceopt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &o.min_cnt, "min k-mer count" },
		{ 's', ARG_I32, &o.min_streak, "min k-mer streak" },
		{ 't', ARG_I32, &o.n_threads, "host threads (accepted for the reference's command line)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per chunk" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("chkerr [options] <count.yak> <seq.fa>", defs, nd); return 1; }
	yak_ch_t *tab = table_load("chkerr", argv[first]);
	if (!tab) return 2;
	const int rc = yakamd_chkerr(&o, tab, argv[first + 1], 0) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- sexchr ---- */
static int cmd_sexchr(int argc, char **argv)
{
	yakamd_scopt_t o;
	yakamd_scopt_init(&o);
	const struct arg_def defs[] = {
		{ 't', ARG_I32, &o.n_threads, "host threads (accepted for the reference's command line)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "chunk size (bases; k, m, g suffixes)" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 4 >= argc) { arg_help("sexchr [options] <chrY.yak> <chrX.yak> <PAR.yak> <hap1.fa> <hap2.fa>", defs, nd); return 1; }
	/* the three loads must agree on k and pre (htab.c:437 asserts it): read the headers before loading anything */
	uint32_t k[3], pre[3];
	for (int i = 0; i < 3; ++i)
		if (!yak_header(argv[first + i], &k[i], &pre[i])) { fprintf(stderr, "yak-amd sexchr: %s is not a readable .yak file\n", argv[first + i]); return 2; }
	for (int i = 1; i < 3; ++i)
		if (k[i] != k[0] || pre[i] != pre[0]) {
			fprintf(stderr, "yak-amd sexchr: %s has k = %u and pre = %u, %s has k = %u and pre = %u: the three tables must agree\n",
			        argv[first], k[0], pre[0], argv[first + i], k[i], pre[i]);
			return 2;
		}
	yak_ch_t *tab = yak_ch_restore_core(0, argv[first], YAK_LOAD_SEXCHR1);
	if (tab) tab = yak_ch_restore_core(tab, argv[first + 1], YAK_LOAD_SEXCHR2);
	if (tab) tab = yak_ch_restore_core(tab, argv[first + 2], YAK_LOAD_SEXCHR3);
	if (!tab) { fprintf(stderr, "yak-amd sexchr: cannot load %s, %s and %s (or no MI355X)\n", argv[first], argv[first + 1], argv[first + 2]); return 2; }
	const int rc = yakamd_sexchr(&o, tab, argv[first + 3], argv[first + 4], 0) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- print ---- */
static int cmd_print(int argc, char **argv)
{
	yakamd_propt_t o;
	int with_counts = 0;
	yakamd_propt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_FLAG, &with_counts, "a tab and the count behind every k-mer" },
		{ 'B', ARG_I64SIZE, &o.batch_bytes, "device bytes of text per range of sub-tables" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first >= argc) { arg_help("print [options] <in.yak>", defs, nd); return 1; }
	if (table_k("print", argv[first], 0, K_32_HASH) < 0) return 2;
	o.with_counts = with_counts;
	yak_ch_t *tab = table_load("print", argv[first]);
	if (!tab) return 2;
	yak_ch_tighten(tab);
	const int rc = yakamd_print(&o, tab, 0) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- cntasm ---- */
static int cmd_cntasm(int argc, char **argv)
{
	yak_copt_t o;
	const char *in = 0, *out = 0;
	int min_cnt = 1, max_cnt = 1, max_out = 0, check_n = 10, pre_resize = 0;   /* reference main.c:94 */
	yak_copt_init(&o);
	o.chunk_size = 1900000000;                               /* -K 1.9g, main.c:98 */
	const struct arg_def defs[] = {
		{ 'k', ARG_I32, &o.k, "k-mer length, below 32" },
		{ 'c', ARG_I32, &min_cnt, "min count in an assembly" },
		{ 'x', ARG_I32, &max_cnt, "max count in an assembly" },
		{ 'p', ARG_I32, &o.pre, "bits of the hash that pick the sub-table" },
		{ 'r', ARG_FLAG, &pre_resize, "resize before merging" },
		{ 't', ARG_I32, &o.n_thread, "host threads (parser)" },
		{ 'e', ARG_I32, &max_out, "drop a k-mer absent from this many assemblies" },
		{ 's', ARG_I32, &check_n, "shrink the table every this many assemblies" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per host batch" },
		{ 'i', ARG_TEXT, &in, "start from this table (.yak); the same name as -o: written over" },
		{ 'o', ARG_TEXT, &out, "write the table (.yak) here" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first >= argc) { arg_help("cntasm [options] <a.fa> [b.fa ...]", defs, nd); return 1; }
	if (o.pre < YAK_COUNTER_BITS || o.k < 1 || o.k >= 32) { fprintf(stderr, "yak-amd cntasm: need 1 <= k < 32 and p >= %d\n", YAK_COUNTER_BITS); return 1; }
	yak_ch_t *tab = 0;
	if (in && !(tab = yak_ch_restore(in))) fprintf(stderr, "yak-amd cntasm: cannot load %s: starting from nothing\n", in);
	for (int i = first; i < argc; ++i) {
		const int done = i - first + 1;
		yak_ch_t *one = yak_count(argv[i], &o, 0);
		if (!one) { fprintf(stderr, "yak-amd cntasm: no table for %s (unreadable input, or no MI355X)\n", argv[i]); yak_ch_destroy(tab); return 2; }
		if (!tab) {
			tab = one;
			yak_ch_shrink(tab, min_cnt, max_cnt, o.n_thread);
			yak_ch_setcnt(tab, 1, o.n_thread);
		} else yak_ch_merge(tab, one, min_cnt, max_cnt, o.n_thread, pre_resize);   /* consumes `one` */
		if (i == argc - 1 || (done > max_out && done % check_n == 0)) yak_ch_shrink(tab, done - max_out, YAK_MAX_COUNT, o.n_thread);   /* main.c:152 */
		fprintf(stderr, "[M::yak-amd] %s done; %ld distinct k-mers in the table\n", argv[i], (long)tab->tot);
	}
	yak_ch_tighten(tab);
	int rc = 0;
	if (out && yak_ch_dump(tab, out) != 0) { fprintf(stderr, "yak-amd cntasm: cannot write %s\n", out); rc = 3; }
	yak_ch_destroy(tab);
	return rc;
}

/* ---- recount ---- */
static int cmd_recount(int argc, char **argv)
{
	const char *out = "-";
	const struct arg_def defs[] = {
		{ 'o', ARG_TEXT, &out, "write the table (.yak) here; - (the default) = stdout" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("recount [options] <in.yak> <seq.fa>", defs, nd); return 1; }
	yak_ch_t *tab = table_load("recount", argv[first]);
	if (!tab) return 2;
	yak_ch_tighten(tab);
	int rc = 0;
	yak_recount(argv[first + 1], tab);
	if (yak_ch_dump(tab, out) != 0) { fprintf(stderr, "yak-amd recount: cannot write %s\n", out); rc = 3; }
	yak_ch_destroy(tab);
	return rc;
}

/* ---- subtract, isec ---- */
/* the first table keeps its k-mers that are absent from (subtract) / present in (isec) every further one */
static int keep_cmd(int argc, char **argv, int isec)
{
	const char *out = "-", *cmd = isec ? "isec" : "subtract";
	int n_thread = 8;                                        /* reference main.c:220 */
	const struct arg_def defs[] = {
		{ 't', ARG_I32, &n_thread, "host threads (accepted for the reference's command line)" },
		{ 'o', ARG_TEXT, &out, "write the table (.yak) here; - (the default) = stdout" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help(isec ? "isec [options] <a.yak> <b.yak> [c.yak ...]" : "subtract [options] <a.yak> <b.yak>", defs, nd); return 1; }
	yak_ch_t *tab = table_load(cmd, argv[first]);
	if (!tab) return 2;
	const int last = isec ? argc : first + 2;
	for (int i = first + 1; i < last; ++i) {
		yak_ch_t *other = yak_ch_restore(argv[i]);
		if (!other) { fprintf(stderr, "yak-amd %s: cannot load %s\n", cmd, argv[i]); yak_ch_destroy(tab); return 2; }
		if (isec) yak_ch_isec(tab, other, n_thread);
		else yak_ch_subtract(tab, other, n_thread);
		yak_ch_destroy(other);
	}
	yak_ch_tighten(tab);
	int rc = 0;
	if (yak_ch_dump(tab, out) != 0) { fprintf(stderr, "yak-amd %s: cannot write %s\n", cmd, out); rc = 3; }
	yak_ch_destroy(tab);
	return rc;
}
static int cmd_subtract(int argc, char **argv) { return keep_cmd(argc, argv, 0); }
static int cmd_isec(int argc, char **argv) { return keep_cmd(argc, argv, 1); }

/* ---- sum (not in the reference) ---- */
/* the first table plus the counts of every further one (yakamd_ch_sum) */
static int cmd_sum(int argc, char **argv)
{
	const char *out = "-";
	int pre_resize = 0;
	const struct arg_def defs[] = {
		{ 'r', ARG_FLAG, &pre_resize, "resize before adding a table" },
		{ 'o', ARG_TEXT, &out, "write the table (.yak) here; - (the default) = stdout" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("sum [options] <a.yak> <b.yak> [c.yak ...]", defs, nd); return 1; }
	yak_ch_t *tab = table_load("sum", argv[first]);
	if (!tab) return 2;
	for (int i = first + 1; i < argc; ++i) {
		yak_ch_t *other = yak_ch_restore(argv[i]);
		if (!other) { fprintf(stderr, "yak-amd sum: cannot load %s\n", argv[i]); yak_ch_destroy(tab); return 2; }
		const int r = yakamd_ch_sum(tab, other, pre_resize);
		yak_ch_destroy(other);
		if (r != 0) { fprintf(stderr, "yak-amd sum: %s: %s\n", argv[i], yakamd_last_error()); yak_ch_destroy(tab); return 3; }
	}
	yak_ch_tighten(tab);
	int rc = 0;
	if (yak_ch_dump(tab, out) != 0) { fprintf(stderr, "yak-amd sum: cannot write %s\n", out); rc = 3; }
	yak_ch_destroy(tab);
	return rc;
}

/* ---- depth (not in the reference) ---- */
/* how often the k-mers of each sequence, or of each window of it, occur in a count table (yakamd_depth) */
static int cmd_depth(int argc, char **argv)
{
	yakamd_dpopt_t o;
	const char *out = 0;
	yakamd_dpopt_init(&o);
	const struct arg_def defs[] = {
		{ 'w', ARG_I64SIZE, &o.window, "k-mer start positions per window; 0 (the default) = one window per sequence" },
		{ 't', ARG_I32, &o.n_threads, "host threads (accepted for symmetry with the other commands)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per chunk" },
		{ 'o', ARG_TEXT, &out, "write the lines here; stdout without it" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("depth [options] <table.yak> <seq.fa>", defs, nd); return 1; }
	if (table_k("depth", argv[first], 0, K_32_LOOKUP) < 0) return 2;
	if (o.window < 0) { fprintf(stderr, "yak-amd depth: -w must not be negative\n"); return 1; }
	yak_ch_t *tab = table_load("depth", argv[first]);
	if (!tab) return 2;
	const int rc = yakamd_depth(&o, tab, argv[first + 1], out) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- cover (not in the reference) ---- */
/* which bases of each sequence lie inside k-mers whose count in a table is within LO:HI, as a table, as intervals or as a masked FASTA (yakamd_cover) */
static int cmd_cover(int argc, char **argv)
{
	yakamd_cvopt_t o;
	const char *out = 0, *range = 0, *mask = 0;
	yakamd_cvopt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_TEXT, &range, "LO[:HI]: a k-mer hits when its count is in LO .. HI, an absent one counting 0; -c N = N:1023 [1:1023]" },
		{ 'b', ARG_FLAG, &o.intervals, "behind each S line its covered intervals as B lines: name, start, end (0-based, half-open)" },
		{ 'm', ARG_TEXT, &mask, "none|soft|hard: write the selected sequences as FASTA instead of the table, covered bases as they are, in lower case or as N (qualities and header comments are not carried)" },
		{ 'f', ARG_F64, &o.min_frac, "select the sequences of which at least this fraction is covered [0]" },
		{ 'n', ARG_I64SIZE, &o.min_hit, "select the sequences with at least this many hitting k-mers [0]" },
		{ 'v', ARG_FLAG, &o.invert, "select the other sequences" },
		{ 't', ARG_I32, &o.n_threads, "host threads (accepted for symmetry with the other commands)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per chunk" },
		{ 'o', ARG_TEXT, &out, "write the output here; stdout without it" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("cover [options] <kmer.yak> <seq.fa>", defs, nd); return 1; }
	if (range) {
		char *end = 0;
		const long a = strtol(range, &end, 10);
		long b = 1023;
		int bad = end == range;
		if (!bad && *end == ':') { const char *q = end + 1; b = strtol(q, &end, 10); bad = end == q; }
		if (bad || *end || a < 0 || b < a || b > 1023) { fprintf(stderr, "yak-amd cover: -c takes LO[:HI] with 0 <= LO <= HI <= 1023\n"); return 1; }
		o.lo = (int32_t)a; o.hi = (int32_t)b;
	}
	if (mask) {
		o.mask = strcmp(mask, "none") == 0 ? 0 : strcmp(mask, "soft") == 0 ? 1 : strcmp(mask, "hard") == 0 ? 2 : -1;
		if (o.mask < 0) { fprintf(stderr, "yak-amd cover: -m takes none, soft or hard\n"); return 1; }
	}
	if (!(o.min_frac >= 0.0 && o.min_frac <= 1.0) || o.min_hit < 0) { fprintf(stderr, "yak-amd cover: -f must be in [0, 1] and -n must not be negative\n"); return 1; }
	if (table_k("cover", argv[first], 0, K_32_LOOKUP) < 0) return 2;
	yak_ch_t *tab = table_load("cover", argv[first]);
	if (!tab) return 2;
	const int rc = yakamd_cover(&o, tab, argv[first + 1], out) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- unitigs (not in the reference) ---- */
/* the de Bruijn graph of a count table's k-mers: its unitigs as FASTA, or with -s its tallies (yakamd_unitigs; with -g yakamd_unitigs_dev of
 * libyak_amd_walk.so, which walks on the GPU as well; with -G yakamd_unitigs_gfa of libyak_amd_gfa.so: the unitigs and the links between them as
 * GFA 1, or with -s the tallies and the G line) */
static int cmd_unitigs(int argc, char **argv)
{
	yakamd_ugopt_t o;
	const char *out = 0;
	int stats = 0, min_cnt = 1, n_threads = 0, on_gpu = 0, gfa = 0;
	yakamd_ugopt_init(&o);
	n_threads = o.n_threads;
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &min_cnt, "a k-mer with a count below this is absent, 1 .. 1023 [1]" },
		{ 's', ARG_FLAG, &stats, "the tallies of the graph and of its unitigs, not the FASTA" },
		{ 't', ARG_I32, &n_threads, "threads of the host walk [8]" },
		{ 'g', ARG_FLAG, &on_gpu, "walk on the GPU too (list ranking over the links); the same text" },
		{ 'G', ARG_FLAG, &gfa, "GFA 1: the unitigs as segments and the links between them (implies -g); with -s a G line more" },
		{ 'o', ARG_TEXT, &out, "write the output here; stdout without it" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first >= argc) { arg_help("unitigs [options] <table.yak>", defs, nd); return 1; }
	if (table_k("unitigs", argv[first], K_ODD_GRAPH, K_32_GRAPH) < 0) return 2;
	if (!min_cnt_ok("unitigs", min_cnt)) return 1;
	if (n_threads < 1) { fprintf(stderr, "yak-amd unitigs: -t must be at least 1\n"); return 1; }
	o.min_cnt = min_cnt; o.stats_only = stats; o.n_threads = n_threads;
	yak_ch_t *tab = table_load("unitigs", argv[first]);
	if (!tab) return 2;
	const int rc = (gfa ? yakamd_unitigs_gfa(&o, tab, out) : on_gpu ? yakamd_unitigs_dev(&o, tab, out) : yakamd_unitigs(&o, tab, out)) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- paths (not in the reference) ---- */
/* the sequences of a file laid onto the unitig graph of a count table: per sequence the unitigs it passes through, in which orientation, from where
 * to where, as GAF, or with -s its tallies (yakamd_paths of libyak_amd_path.so) */
static int cmd_paths(int argc, char **argv)
{
	yakamd_ppopt_t o;
	const char *out = 0;
	int stats = 0, min_cnt = 1, min_len = 0;
	yakamd_ppopt_init(&o);
	min_len = o.min_len;
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &min_cnt, "a k-mer with a count below this is absent, 1 .. 1023 [1]" },
		{ 'l', ARG_I32, &min_len, "write the paths that cover at least this many bases of their sequence [k: all of them]" },
		{ 's', ARG_FLAG, &stats, "per sequence its k-mers, hits, paths and steps, not the paths" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per device chunk; a sequence is never cut" },
		{ 'o', ARG_TEXT, &out, "write the output here; stdout without it" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("paths [options] <table.yak> <seqs.fa|fq[.gz]>", defs, nd); return 1; }
	if (table_k("paths", argv[first], K_ODD_GRAPH, K_32_GRAPH) < 0) return 2;
	if (!min_cnt_ok("paths", min_cnt)) return 1;
	if (min_len < 0 || o.chunk_size < 1) { fprintf(stderr, "yak-amd paths: -l must not be negative and -K must be at least 1\n"); return 1; }
	o.min_cnt = min_cnt; o.min_len = min_len; o.stats_only = stats;
	yak_ch_t *tab = table_load("paths", argv[first]);
	if (!tab) return 2;
	const int rc = yakamd_paths(&o, tab, argv[first + 1], out) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- bubbles (not in the reference) ---- */
/* the simple bubbles of the unitig graph of a count table -- a fork whose two arms are one unitig each and join again --, a line per bubble with
 * its type (SNP, equal length, indel) and its two alleles, or with -s the tallies of `unitigs -G -s` and a B line (yakamd_bubbles of
 * libyak_amd_bubble.so).  With -r the reads of a file are laid onto the graph and every bubble gets the reads that pass its two alleles: the
 * support and a call per bubble, with -f the alleles every read passes (yakamd_alleles of libyak_amd_allele.so); with -p as well the alleles
 * are phased from the reads that span two bubbles: a haplotype per het bubble and the blocks (yakamd_phase of libyak_amd_phase.so) */
static int cmd_bubbles(int argc, char **argv)
{
	yakamd_ugopt_t o;
	yakamd_alopt_t a;
	yakamd_phopt_t p;
	const char *out = 0, *reads = 0;
	int stats = 0, min_cnt = 1, frags = 0, phase = 0, edges = 0;
	int32_t min_sup = INT32_MIN, min_frag = INT32_MIN, min_link = INT32_MIN;           /* not given */
	yakamd_ugopt_init(&o);
	yakamd_alopt_init(&a);
	yakamd_phopt_init(&p);
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &min_cnt, "a k-mer with a count below this is absent, 1 .. 1023 [1]" },
		{ 's', ARG_FLAG, &stats, "the tallies of the graph, its unitigs and links, and of the bubbles, forks and tips, not the bubbles" },
		{ 'o', ARG_TEXT, &out, "write the output here; stdout without it" },
		{ 'r', ARG_TEXT, &reads, "reads (fa|fq[.gz]): per bubble the reads that pass each allele and a call, not the bubbles; -s: their tallies" },
		{ 'm', ARG_I32, &min_sup, "with -r: an allele is supported by this many reads that span it [2]" },
		{ 'n', ARG_I32, &min_frag, "with -r -f: list the reads that span this many alleles or more [1]" },
		{ 'f', ARG_FLAG, &frags, "with -r: an F line per read with the alleles it spans" },
		{ 'p', ARG_FLAG, &phase, "with -r: phase the alleles from the reads that span two bubbles: a haplotype per het bubble, and the blocks" },
		{ 'w', ARG_I32, &min_link, "with -r -p: two bubbles are linked from this many votes more one way than the other [2]" },
		{ 'e', ARG_FLAG, &edges, "with -r -p: an E line per link with its votes" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first >= argc) { arg_help("bubbles [options] <table.yak>", defs, nd); return 1; }
	if (!reads && (min_sup != INT32_MIN || min_frag != INT32_MIN || frags)) { fprintf(stderr, "yak-amd bubbles: -m, -n and -f need the reads of -r\n"); return 1; }
	if (!reads && (phase || min_link != INT32_MIN || edges)) { fprintf(stderr, "yak-amd bubbles: -p, -w and -e need the reads of -r\n"); return 1; }
	if (!phase && (min_link != INT32_MIN || edges)) { fprintf(stderr, "yak-amd bubbles: -w and -e need the phasing of -p\n"); return 1; }
	if (phase && (frags || min_frag != INT32_MIN)) { fprintf(stderr, "yak-amd bubbles: -f and -n do not go with -p, which keeps the fragments on the device\n"); return 1; }
	if (table_k("bubbles", argv[first], K_ODD_GRAPH, K_32_GRAPH) < 0) return 2;
	if (!min_cnt_ok("bubbles", min_cnt)) return 1;
	if (min_sup == INT32_MIN) min_sup = a.min_sup;
	if (min_frag == INT32_MIN) min_frag = a.min_frag;
	if (min_link == INT32_MIN) min_link = p.min_link;
	if (min_sup < 1 || min_frag < 1) { fprintf(stderr, "yak-amd bubbles: -m and -n must be at least 1\n"); return 1; }
	if (min_link < 1) { fprintf(stderr, "yak-amd bubbles: -w must be at least 1\n"); return 1; }
	o.min_cnt = min_cnt; o.stats_only = stats;
	yak_ch_t *tab = table_load("bubbles", argv[first]);
	if (!tab) return 2;
	int rc;
	if (reads && phase) {
		p.min_cnt = min_cnt; p.min_sup = min_sup; p.min_link = min_link; p.edges = edges; p.stats_only = stats;
		rc = yakamd_phase(&p, tab, reads, out) == 0 ? 0 : 3;
	} else if (reads) {
		a.min_cnt = min_cnt; a.min_sup = min_sup; a.min_frag = min_frag; a.fragments = frags; a.stats_only = stats;
		rc = yakamd_alleles(&a, tab, reads, out) == 0 ? 0 : 3;
	} else
		rc = yakamd_bubbles(&o, tab, out) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- clean (not in the reference) ---- */
/* the unitig graph of a count table cleaned round by round -- tips clipped, the weaker arm of every simple bubble popped -- by taking the k-mers of
 * the removed unitigs out of the table: the cleaned table goes to a .yak file that every command reads (yakamd_clean of libyak_amd_clean.so) */
static int cmd_clean(int argc, char **argv)
{
	yakamd_cleanopt_t o;
	const char *report = 0;
	int list = 0;
	yakamd_cleanopt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &o.min_cnt, "a k-mer with a count below this is absent and is dropped, 1 .. 1023 [1]" },
		{ 't', ARG_I32, &o.tip_nodes, "clip tips of fewer nodes than this, 0 .. 1048576, 0: none [k]" },
		{ 'b', ARG_I32, &o.pop_pct, "pop the weaker arm of a bubble when its coverage is at most this per cent of the other's, 0 .. 100, 0: none [100]" },
		{ 'r', ARG_I32, &o.max_rounds, "rounds at the most, 1 .. 64 [8]" },
		{ 'l', ARG_FLAG, &list, "list every removed unitig in the report (T and P lines)" },
		{ 'o', ARG_TEXT, &report, "write the report here; stdout without it" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("clean [options] <in.yak> <out.yak>", defs, nd); return 1; }
	if (table_k("clean", argv[first], K_ODD_GRAPH, K_32_GRAPH) < 0) return 2;
	if (!min_cnt_ok("clean", o.min_cnt)) return 1;
	if (o.tip_nodes < -1 || o.tip_nodes > YAKAMD_CLEAN_MAX_TIP_NODES || o.pop_pct < 0 || o.pop_pct > 100 || o.max_rounds < 1 || o.max_rounds > 64) {
		fprintf(stderr, "yak-amd clean: -t must be in [0, %d], -b in [0, 100] and -r in [1, 64]\n", YAKAMD_CLEAN_MAX_TIP_NODES);
		return 1;
	}
	o.list = list;
	yak_ch_t *tab = table_load("clean", argv[first]);
	if (!tab) return 2;
	const int rc = yakamd_clean(&o, tab, argv[first + 1], report ? report : "-") == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- correct (not in the reference) ---- */
/* the reads with their single substitution errors repaired against a count table: a run of weak k-mers whose length names the base, the three
 * other bases tried with the table's own lookup, the base replaced where exactly one of them makes the run solid (yakamd_correct of
 * libyak_amd_correct.so) */
static int cmd_correct(int argc, char **argv)
{
	yakamd_cropt_t o;
	const char *out = 0, *report = 0;
	yakamd_cropt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &o.min_cnt, "a k-mer with a count below this is weak, 1 .. 1023 [3]" },
		{ 'e', ARG_I32, &o.min_run, "the shortest run of weak k-mers that is tried, 1 .. k [1]" },
		{ 'l', ARG_FLAG, &o.list, "list every fixed base in the report (X lines)" },
		{ 's', ARG_FLAG, &o.stats_only, "the report alone: no reads are written (the report goes to stdout without -r)" },
		{ 'K', ARG_I64SIZE, &o.chunk_size, "bases per chunk" },
		{ 'o', ARG_TEXT, &out, "write the corrected reads here; stdout without it" },
		{ 'r', ARG_TEXT, &report, "write the report here; none without it" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first + 1 >= argc) { arg_help("correct [options] <kmer.yak> <reads.fq>", defs, nd); return 1; }
	const int k = table_k("correct", argv[first], 0, K_32_LOOKUP);
	if (k < 0) return 2;
	if (!min_cnt_ok("correct", o.min_cnt)) return 1;
	if (o.min_run < 1 || o.min_run > k) { fprintf(stderr, "yak-amd correct: -e must be in [1, %d], the table's k\n", k); return 1; }
	if (o.chunk_size < 1) { fprintf(stderr, "yak-amd correct: -K must be in [1, 2^63)\n"); return 1; }
	yak_ch_t *tab = table_load("correct", argv[first]);
	if (!tab) return 2;
	const int rc = yakamd_correct(&o, tab, argv[first + 1], out, report ? report : o.stats_only ? "-" : 0) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- hetmers (not in the reference) ---- */
/* the pairs of k-mers of a count table that differ in the middle base alone, as a histogram of their two counts (yakamd_hetmers) */
static int cmd_hetmers(int argc, char **argv)
{
	yakamd_hmopt_t o;
	const char *out = 0;
	int pairs = 0, min_cnt = 1;
	yakamd_hmopt_init(&o);
	const struct arg_def defs[] = {
		{ 'c', ARG_I32, &min_cnt, "a k-mer with a count below this is absent, 1 .. 1023 [1]" },
		{ 'p', ARG_FLAG, &pairs, "list the pairs themselves (K lines)" },
		{ 'o', ARG_TEXT, &out, "write the lines here; stdout without it" },
	};
	const int nd = (int)(sizeof(defs) / sizeof(defs[0]));
	const int first = arg_scan(argc, argv, defs, nd);
	if (first < 0 || first >= argc) { arg_help("hetmers [options] <table.yak>", defs, nd); return 1; }
	if (table_k("hetmers", argv[first], K_ODD_MIDDLE, K_32_GRAPH) < 0) return 2;
	if (!min_cnt_ok("hetmers", min_cnt)) return 1;
	o.min_cnt = min_cnt; o.print_pairs = pairs;
	yak_ch_t *tab = table_load("hetmers", argv[first]);
	if (!tab) return 2;
	const int rc = yakamd_hetmers(&o, tab, out) == 0 ? 0 : 3;
	yak_ch_destroy(tab);
	return rc;
}

/* ---- version ---- */
static int cmd_version(int argc, char **argv)
{
	(void)argc; (void)argv;
	puts(YAKS_VERSION);
	return 0;
}

int main(int argc, char **argv)
{
	static const struct { const char *name; int (*run)(int, char**); int beyond; const char *what; } cmds[] = {   /* beyond: not in the reference */
		{ "count", cmd_count, 0, "count k-mers on the GPU, write a .yak table" },
		{ "qv", cmd_qv, 0, "look the k-mers of sequences up in a .yak table" },
		{ "triobin", cmd_triobin, 0, "bin reads by the k-mers of the two parents' .yak tables" },
		{ "trioeval", cmd_trioeval, 0, "evaluate the phasing of an assembly by the k-mers of the two parents' .yak tables" },
		{ "inspect", cmd_inspect, 0, "the k-mer histogram of a .yak table, or the joint spectrum of two" },
		{ "chkerr", cmd_chkerr, 0, "report the streaks of low k-mers of sequences against a .yak table" },
		{ "sexchr", cmd_sexchr, 0, "count the sex-chromosome k-mers of two haplotype assemblies" },
		{ "print", cmd_print, 0, "list the k-mers of a .yak table as text" },
		{ "cntasm", cmd_cntasm, 0, "count in how many assemblies each k-mer occurs, write a .yak table" },
		{ "recount", cmd_recount, 0, "count the k-mers of a .yak table in other sequences" },
		{ "subtract", cmd_subtract, 0, "the k-mers of a .yak table that are absent from a second one" },
		{ "isec", cmd_isec, 0, "the k-mers of a .yak table that are present in every further one" },
		{ "version", cmd_version, 0, "print the version" },
		{ "sum", cmd_sum, 1, "add the counts of two or more .yak tables together" },
		{ "depth", cmd_depth, 1, "the depth of the k-mers of each sequence, or window, in a .yak table" },
		{ "hetmers", cmd_hetmers, 1, "the pairs of k-mers of a .yak table that differ in the middle base, by their two counts" },
		{ "cover", cmd_cover, 1, "the bases of each sequence that lie inside k-mers a .yak table holds, lacks or holds too often" },
		{ "unitigs", cmd_unitigs, 1, "the unitigs of the de Bruijn graph that the k-mers of a .yak table span" },
		{ "paths", cmd_paths, 1, "sequences as paths through the unitigs of that graph (GAF)" },
		{ "bubbles", cmd_bubbles, 1, "the simple bubbles of that graph: forks whose two arms join again, with their alleles" },
		{ "clean", cmd_clean, 1, "that graph with its tips clipped and its bubbles popped, as a .yak table of the k-mers that stay" },
		{ "correct", cmd_correct, 1, "reads with their single substitution errors repaired against a .yak table" },
	};
	const size_t n_cmds = sizeof(cmds) / sizeof(cmds[0]);
	/* -X name=value (anywhere on the line, any number of times): a test switch of the library (yakamd_test_set) -- tests force code paths with it */
	for (int i = 1; i + 1 < argc; ) {
		char *eq = strcmp(argv[i], "-X") == 0 ? strchr(argv[i + 1], '=') : 0;
		if (!eq) { ++i; continue; }
		*eq = 0;
		yakamd_test_set(argv[i + 1], atoll(eq + 1));
		memmove(argv + i, argv + i + 2, (size_t)(argc - i - 2) * sizeof(char*));
		argc -= 2;
	}
	if (argc >= 2)
		for (size_t i = 0; i < n_cmds; ++i)
			if (strcmp(argv[1], cmds[i].name) == 0) return cmds[i].run(argc - 1, argv + 1);
	fprintf(stderr, "yak-amd: driver of libyak_amd.so (lh3/yak's C API on MI355X)\n");
	for (size_t i = 0; i < n_cmds; ++i) {
		if (cmds[i].beyond && !cmds[i - 1].beyond) fprintf(stderr, "  beyond the reference:\n");
		fprintf(stderr, "%s    yak-amd %-8s %s\n", cmds[i].beyond ? "  " : "", cmds[i].name, cmds[i].what);
	}
	return 1;
}
