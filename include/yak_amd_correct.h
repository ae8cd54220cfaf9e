/* yak_amd_correct.h -- single substitution errors of reads repaired on the GPU against a count table (libyak_amd_correct.so; not in the reference;
 * DESIGN.md section 30).  A layer above libyak_amd.so alone: the table is looked up with yakamd_lookup_dev(), nothing else of it is touched.
 *
 * Inputs.  The image is a base image as yakamd_lookup_dev() takes it (16-byte aligned, room for n_bytes rounded up to 16).  Sequence j is the bytes
 * [off[j], off[j] + len[j]), followed by '\n'; the sequences ascend and are disjoint.  cnt[i] is that call's output: the count of the canonical
 * k-mer ENDING at byte i, or 0xffff where none ends.  c = min_cnt >= 1.
 *
 * Per-position terms.  Position i EXISTS iff cnt[i] != 0xffff (a position in front of the image or behind it does not).  It is WEAK iff it exists
 * and cnt[i] < c -- an absent k-mer counts 0, so it is weak.  It is SOLID iff it exists and is not weak.
 *
 * Candidates.  A RUN is a maximal [st, en) of consecutive weak positions, given relative to the sequence; no run crosses a non-base.  A run is a
 * CANDIDATE iff en - st >= min_run and one of
 *   en - st == k: the base is p = st;
 *   en - st <  k, st - 1 does not exist and en exists (the first k-mers of a stretch of bases): p = en - k;
 *   en - st <  k, en does not exist and st - 1 exists (the last k-mers of a stretch): p = st.
 * Nothing else is a candidate: runs longer than k (errors closer than k), short runs with both neighbours solid, short runs with neither
 * neighbour existing.  By construction the k-mers that contain base p are exactly those ending in [st, en).  (On an array that no lookup wrote
 * en - k can lie in front of the sequence: such a run is no candidate either.)
 *
 * Trials.  o = seq_nt4_table[byte at p].  The three codes b != o, ascending, are tried: trial b FITS iff, with the byte at p replaced, every k-mer
 * ending in [st, en) is solid.  The candidate is FIXED iff exactly one trial fits: the byte becomes "ACGT"[b], in lower case iff the original byte
 * has bit 0x20 set.  Otherwise it is AMBIGUOUS (two or three trials fit) or has NO FIT; the read keeps its base in both cases.
 *
 * Consequences.  The runs of two candidates are disjoint and no k-mer of one candidate's run contains the other's p, so all decisions are taken on
 * one snapshot, applied together, and depend on no order.  The corrected image's weak positions are exactly the old ones minus the fixed runs:
 * n_weak_after = n_weak - the sum of en - st over the fixed candidates.  A second correction of the corrected reads fixes nothing and reports the
 * same ambiguous and no-fit candidates.
 *
 * Refused (message, -1 or NULL, before any device work where the cause is in the arguments): everything yakamd_lookup_dev() refuses -- k >= 32, a
 * sharded table, a table on several devices, an open pass; a table marked homopolymer-compressed (yakamd_ch_hpc); min_cnt outside [1, 1023];
 * min_run outside [1, k]; chunk_size < 1; an input that cannot be opened, refused before either output is created.
 *
 * The device-level calls.  All pointers are the caller's device memory and 16-byte aligned; cap is in entries or bytes; with a NULL output or a
 * smaller cap a call returns the number needed and writes no record.  -1 after a message (yakamd_correct_last_error()).  Each returns when the
 * device is done.
 *   yakamd_correct_find_dev()    the candidates of cnt[0 .. n_bytes) in image order into d_fix: at = the image byte of the base, seq, p, st, en; from,
 *                                to, fit, why and reserved are 0.  d_tally[0 .. n_seq) (NULL: none) is overwritten, in the counting call too: n_kmer
 *                                (positions that exist), n_weak, n_cand, n_weak_after = n_weak, 0 elsewhere.  n_bytes = 0 launches nothing.
 *   yakamd_correct_trials_dev()  the trial image of the n_fix records: trial t = 3 cand + a, a the rank of the code among the three, is bytes
 *                                [2k t, 2k (t + 1)): the image bytes [off + st - k + 1, off + en) with byte `at` replaced by the upper-case base,
 *                                then '\n' to the end of the stride; the whole is padded with '\n' to a multiple of 16.  Returns its size,
 *                                up16(6 k n_fix).  A record that does not lie inside the image, or whose byte is no base, is refused.
 *   yakamd_correct_decide_dev()  d_trial_cnt is yakamd_lookup_dev()'s output on the trial image.  Per record: from = the byte at `at`, fit has bit b
 *                                set iff trial b fits, why = YAKAMD_FIX_*, to = the byte written or 0; the byte is written into d_bases; n_fixed,
 *                                n_ambig and n_nofit are added to d_tally[seq] and en - st of a fixed record is taken from its n_weak_after.
 *   yakamd_correct_image_dev()   lookup, find, trials, lookup and decide on one image in place; returns the number of candidates, their records in
 *                                d_fix when cap suffices -- the image is corrected and the tallies are complete either way.  An image without
 *                                candidates launches neither the trials nor the decisions nor the second lookup. */
#ifndef YAK_AMD_CORRECT_H
#define YAK_AMD_CORRECT_H
#include "yak_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t at; uint32_t seq, p, st, en; uint8_t from, to, fit, why; uint32_t reserved; } yakamd_fix_t;     /* 32 bytes */
typedef struct { uint32_t n_kmer, n_weak, n_cand, n_fixed, n_ambig, n_nofit, n_weak_after, reserved; } yakamd_ctally_t;   /* 32 bytes */
enum { YAKAMD_FIX_NOFIT = 0, YAKAMD_FIX_DONE = 1, YAKAMD_FIX_AMBIG = 2 };
typedef struct {
	int32_t min_cnt;          /* -c, 3 (chkerr's): a k-mer below this count is weak */
	int32_t min_run;          /* -e, 1: the shortest run that is tried */
	int32_t list;             /* -l, 0: an X line per fixed base */
	int32_t stats_only;       /* -s, 0: no reads are written */
	int64_t chunk_size;       /* -K, 1 << 28: bases per chunk; a sequence is never cut */
} yakamd_cropt_t;
void yakamd_cropt_init(yakamd_cropt_t *o);

int64_t yakamd_correct_find_dev(int k, int min_cnt, int min_run, const void *d_cnt_u16, int64_t n_bytes, const uint64_t *d_seq_off,
                                const uint32_t *d_seq_len, int64_t n_seq, yakamd_fix_t *d_fix, int64_t cap, yakamd_ctally_t *d_tally);
int64_t yakamd_correct_trials_dev(int k, const void *d_bases, int64_t n_bytes, const yakamd_fix_t *d_fix, int64_t n_fix, void *d_trials, int64_t cap_bytes);
int     yakamd_correct_decide_dev(int k, int min_cnt, const void *d_trial_cnt_u16, yakamd_fix_t *d_fix, int64_t n_fix, void *d_bases, int64_t n_bytes,
                                  yakamd_ctally_t *d_tally, int64_t n_seq);
int64_t yakamd_correct_image_dev(yak_ch_t *h, int min_cnt, int min_run, void *d_bases, int64_t n_bytes, const uint64_t *d_seq_off,
                                 const uint32_t *d_seq_len, int64_t n_seq, yakamd_fix_t *d_fix, int64_t cap, yakamd_ctally_t *d_tally);

/* `yak-amd correct` as a library call: every record of `fn` (FASTA / FASTQ, .gz, "-" = stdin) against `ch`, a YAK_LOAD_ALL table (yak_ch_restore)
 * or a resident one.  The reads go to out_fn (NULL or "-": stdout; not written with stats_only) in input order, the sequence on one line:
 * `>name[ comment]\nSEQ\n` without a quality, `@name[ comment]\nSEQ\n+\nQUAL\n` with one; a record whose sequence needs no change leaves byte-equal
 * to that normal form.  The report goes to report_fn (NULL: none; "-": stdout), tabs between the fields:
 *   `#correct k=<k> min_cnt=<c> min_run=<e>`
 *   `S name len n_kmer n_weak n_cand n_fixed n_ambig n_nofit n_weak_after` per sequence
 *   with list, behind each S line in position order: `X name p from to run_len`
 *   `T n_seq sum_len` and the seven sums, last
 * Neither text depends on chunk_size.  0, or -1 after a message. */
int     yakamd_correct(const yakamd_cropt_t *o, yak_ch_t *ch, const char *fn, const char *out_fn, const char *report_fn);
/* measurement: the milliseconds the calling thread's last yakamd_correct_image_dev / yakamd_correct call spent on the first lookup, the find, the
 * trials, the second lookup, the decisions and the text (with the reader and the copies) */
void    yakamd_correct_ms(double ms[6]);
const char *yakamd_correct_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_clean_tally_names / _read / _reset are for libyak_amd_clean.so's */
int  yakamd_correct_tally_names(const char *const **names);
void yakamd_correct_tally_read(uint64_t *out, int n);
void yakamd_correct_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
