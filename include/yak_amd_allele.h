/* yak_amd_allele.h -- the alleles of the simple bubbles supported with reads, on the GPU (libyak_amd_allele.so; not in the reference; DESIGN.md
 * section 31).
 *
 * A layer above libyak_amd_path.so, libyak_amd_bubble.so, libyak_amd_gfa.so, libyak_amd_walk.so and libyak_amd.so: it joins the path records and
 * steps of include/yak_amd_path.h (section 23) with the bubble records of include/yak_amd_bubble.h (section 26), and nothing else.  An oriented
 * unitig is j << 1 | o (o = 1 for '-'); a step, a path and a hit are what the path header defines; a bubble record is (src, sink, arm[2], ...) with
 * its index i in list order.
 *
 * Arm map: unitig j is an arm iff arm[a] >> 1 == j for some bubble i and a in {0, 1}; then arm_of[j] = i << 1 | a.  An arm belongs to one bubble
 * alone; every other unitig maps to ~0.
 * Observation: a step j << 1 | o of a path with arm_of[j] != ~0 is an observation of allele a of bubble i.  It is full iff its step is neither the
 * first nor the last step of its path, partial otherwise.  Consecutive steps of a path are links and an arm has one link on either side, so a full
 * observation has src before it and sink behind it (sink ^ 1 before and src ^ 1 behind for rev): the read holds the whole allele with a base of
 * flank on either side.  rev = o ^ (arm[a] & 1): with rev = 0 the read passes the bubble from source to sink.
 * Record: yakamd_aobs_t, 16 bytes; flags bit 0 is a, bit 1 full, bit 2 rev; seq and path index the chunk's d_seq_off and d_paths.  The records are
 * in step order, which is image order.
 * Support: yakamd_asup_t per bubble, 32 bytes: the observations counted over everything fed since the open or the last reset.  A read that passes
 * an arm twice -- twice round a circle -- counts twice.
 * Call: with min_sup = m in [1, 2^31), allele a is supported iff full[a] >= m; the call is het (both), hom1, hom2 or none.  Integers only.
 *
 * yakamd_allele_open(): borrows the walk and the bubbles; the number of unitigs is the walk's, a copy of the records is taken through
 * yakamd_bubble_records_dev(), arm_of[] is built and the support set to zero; all of it stays in device memory until yakamd_allele_close().  The
 * device current at the call is used and stays current, here and in every call below; all device pointers are the caller's.  NULL after a message
 * (yakamd_allele_last_error()), before any device work: w or b is NULL; the walk has 2^31 unitigs or more; there are 2^31 bubbles or more.  NULL as
 * well, after the kernel, for a record whose arm names no unitig of the walk and for a unitig that two arms claim: such a record is counted and
 * reported, and decides nothing.  A genuine set of bubbles never claims a unitig twice: YAKAMD_ALLELE_DAMAGE=dup, a test switch read from the
 * environment, makes the second arm of the last record the first arm of the first, to show that refusal on a device.  Zero bubbles open, and
 * nothing is ever observed.
 * yakamd_allele_obs_dev(): d_paths[0 .. n_path) and d_steps[0 .. n_step) as yakamd_path_chain_dev() wrote them (16-byte and 8-byte aligned), d_obs
 * 16-byte aligned, cap in entries.  Always writes n_out = { n_obs, n_full }.  0 when the records were written -- only then are they added to the
 * support --, 1 when it has only counted (d_obs is NULL or cap too small; the support is untouched), -1 after a message.  With n_step = 0 it
 * launches nothing.  Every index read from device data is checked before it is used: a step's unitig against the walk, a path's
 * [step_off, step_off + n_step) against n_step and against the path before it; a misfit is counted and the call returns -1.
 * yakamd_allele_support_dev() copies the n_bubble entries into device memory of the caller (cap in entries, 16-byte aligned) and returns their
 * number; with a NULL pointer or a smaller cap the number needed, and nothing is written.  -1 after a message.
 * yakamd_allele_reset() sets the support back to zero. */
#ifndef YAK_AMD_ALLELE_H
#define YAK_AMD_ALLELE_H
#include "yak_amd_path.h"
#include "yak_amd_bubble.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { YAKAMD_AOBS_A = 1, YAKAMD_AOBS_FULL = 2, YAKAMD_AOBS_REV = 4 };

typedef struct yakamd_allele yakamd_allele_t;
typedef struct { uint32_t seq, bubble, flags, path; } yakamd_aobs_t;      /* 16 bytes */
typedef struct { uint64_t full[2], part[2]; } yakamd_asup_t;             /* 32 bytes */
typedef struct { uint64_t n_unitig, n_bubble, n_arm; } yakamd_alstat_t;
typedef struct {
	int32_t min_cnt;      /* a k-mer with a count below this is absent, 1 .. 1023 [1] */
	int32_t min_sup;      /* an allele is supported by this many full observations, 1 .. 2^31 - 1 [2] */
	int32_t min_frag;     /* an F line for a read with this many full observations, 1 .. 2^31 - 1 [1] */
	int32_t fragments;    /* 1: the observation records are copied out, the reads with min_frag full observations counted and their F lines written */
	int32_t stats_only;   /* the header and the T line only */
	int32_t reserved;
	int64_t chunk_size;   /* bases per device chunk; a sequence is never cut [1 << 28] */
} yakamd_alopt_t;
void yakamd_alopt_init(yakamd_alopt_t *o);

yakamd_allele_t *yakamd_allele_open(yakamd_uwalk_t *w, yakamd_bubble_set_t *b);      /* borrows both; arm_of, the records and the support stay on the device until close */
int     yakamd_allele_stats(yakamd_allele_t *al, yakamd_alstat_t *st);
int     yakamd_allele_obs_dev(yakamd_allele_t *al, const yakamd_upath_t *d_paths, int64_t n_path, const uint64_t *d_steps, int64_t n_step,
                              yakamd_aobs_t *d_obs, int64_t cap, int64_t n_out[2]);
int64_t yakamd_allele_support_dev(yakamd_allele_t *al, void *d, int64_t cap);       /* n_bubble entries of yakamd_asup_t */
int     yakamd_allele_reset(yakamd_allele_t *al);
void    yakamd_allele_close(yakamd_allele_t *al);

/* `yak-amd bubbles -r` as a library call: the walk at min_cnt, the links, the bubbles, the arm map and the index of the paths; the walk, the links
 * and the bubbles closed; then the reads of reads_fn (FASTA or FASTQ, plain or gzip, `-` for stdin) in chunks: upload, hits, chain, observations.
 * The text, tab-separated, does not depend on chunk_size:
 *   #alleles k=<k> min_cnt=<c> min_sup=<m>
 *   F <name> <n> <i>:<1|2><+|-> ...     with fragments: per read, in input order, with n >= min_frag full observations, those in read order; + for
 *                                       rev = 0
 *   A <i> u<a1><+|-> u<a2><+|-> <full1> <full2> <part1> <part2> <het|hom1|hom2|none>     per bubble, i and the u<j> as in `yak-amd bubbles`
 *   T n_seq sum_len n_path n_step n_obs n_full n_frag n_bubble n_het n_hom1 n_hom2 n_none
 * n_frag = the reads with min_frag full observations or more; they are counted from the records, so without fragments it is 0.  With stats_only
 * the header and the T line only.  0, or -1 after a message on stderr -- on a refusal before the output is created: everything yakamd_uwalk_open(),
 * yakamd_gfa_open(), yakamd_bubble_open(), yakamd_allele_open() and yakamd_path_open() refuse, a table marked homopolymer-compressed, reads that
 * cannot be opened, min_sup < 1, min_frag < 1, chunk_size < 1 */
int     yakamd_alleles(const yakamd_alopt_t *o, yak_ch_t *ch, const char *reads_fn, const char *out_fn);
/* measurement: the milliseconds the calling thread's last yakamd_allele_open / yakamd_alleles call spent on the arm map and, summed over the
 * chunks, on the count and the scan, the emit, the copies, the text; yakamd_allele_open() sets all five back, and every later
 * yakamd_allele_obs_dev() of the thread adds to its part */
void    yakamd_allele_ms(double ms[5]);
const char *yakamd_allele_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_gfa_tally_names / _read / _reset are for libyak_amd_gfa.so's */
int  yakamd_allele_tally_names(const char *const **names);
void yakamd_allele_tally_read(uint64_t *out, int n);
void yakamd_allele_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
