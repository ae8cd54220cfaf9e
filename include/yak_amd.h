/*
 * yak_amd.h -- device-level entry points of the MI355X counting engine (C ABI, plain pointers).
 *
 * yak.h is the drop-in surface; the functions below are what yak_count()/yak_ch_*() are built
 * from, exported so that a harness can (a) hand over bases that are ALREADY resident in HBM,
 * (b) time the device path without host parsing / PCIe, and (c) shard the sub-tables over several
 * GPUs.  No torch types, no C++ types: `void *` device pointers and sizes only.
 *
 * Input format ("base image"): ASCII sequence bytes; every byte that is not one of
 * A C G T U a c g t u or a raw 0..3 (reference misc.c:4-21) breaks the rolling k-mer exactly like
 * an 'N' or a record boundary does in reference count.c:41, so sequences are simply separated by
 * at least one such byte (e.g. '\n').
 */
#ifndef YAK_AMD_H
#define YAK_AMD_H

#include <stdint.h>
#include <stddef.h>
#include "yak.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yakamd_ctx yakamd_ctx;        /* device state behind one yak_ch_t */

/* number of usable gfx950 devices (0 if none); never falls back to the CPU */
int yakamd_device_count(void);
/* last error message of the calling thread ("" if none) */
const char *yakamd_last_error(void);

/* engine bound to an existing table (the yak_ch_t returned by yak_ch_init) */
yakamd_ctx *yakamd_ctx_of(yak_ch_t *h);
/* restrict the engine to the sub-tables [lo, hi): k-mers of other prefixes are dropped at
 * insertion (multi-GPU prefix sharding, replaces the kt_for over prefixes of count.c:133) */
int yakamd_set_shard(yak_ch_t *h, int prefix_lo, int prefix_hi);

/* One counting pass = begin, any number of feeds, end  (replaces count.c:85-166).
 * create_new as in yak_ch_insert_list (htab.c:51).  `t0` = position of the first byte of this
 * buffer in the logical input stream (stream order decides the table layout). */
int yakamd_pass_begin(yak_ch_t *h, int create_new);
int yakamd_feed_bases_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, uint64_t t0);
int yakamd_feed_bases_host(yak_ch_t *h, const void *h_bases, int64_t n_bytes, uint64_t t0);
/* the same stream packed to 0.375 bytes per base (what count.c:28-43 keeps of a base: its 2-bit code, or "not ACGT"): d_codes =
 * 32-bit words of 16 bases, base j of the stream at bits 2 (j % 16) of word j / 16, code = seq_nt4_table (A 0, C 1, G 2, T 3);
 * d_valid = one bit per base, bit j % 32 of word j / 32, 0 for N / any other byte / the separator between two records.
 * Both device pointers, the codes 16-byte aligned; words past n_bases are not read beyond the last partial one.  The counting
 * passes then read 0.375 B per position instead of 1 */
int yakamd_feed_packed_dev(yak_ch_t *h, const void *d_codes, const void *d_valid, int64_t n_bases, uint64_t t0);
/* the packed image from host memory: `h_packed` = yakamd_packed_bytes(n_bases) bytes, the code words followed (at the next multiple of 16
 * bytes) by the validity words -- what yakamd_pack_bases_host() writes (any thread; yak_count()'s parser threads pack what they parsed,
 * so the stream crosses the bus at 0.375 B per base, count.c:88-110's reader loop being the host side of this) */
int64_t yakamd_packed_bytes(int64_t n_bases);
void yakamd_pack_bases_host(const void *ascii, int64_t n_bases, void *h_packed);
int yakamd_feed_packed_host(yak_ch_t *h, const void *h_packed, int64_t n_bases, uint64_t t0);
/* ... or as pieces, each a whole number of 32-position words (n_words[i] validity words at valid[i], twice as many code words at codes[i]; a
 * piece whose bases end inside its last word leaves the rest of it invalid): laid one behind the other on the device, fed as ONE image of
 * 32 * sum(n_words) stream positions.  yak_count() hands over a window of its parser's segments this way (stream positions only order the
 * k-mers: the up to 31 unused ones behind a segment change nothing) */
int yakamd_feed_packed_pieces_host(yak_ch_t *h, int n_pieces, const void *const *codes, const void *const *valid, const int64_t *n_words, uint64_t t0);
/* device-side packer: ASCII image -> d_codes ((n + 31) / 32 * 8 bytes) and d_valid ((n + 31) / 32 * 4 bytes); `stream` = a hipStream_t or 0 */
int yakamd_pack_bases_dev(const void *d_ascii, int64_t n, void *d_codes, void *d_valid, void *stream);
/* already hashed k-mers (yak_hash64 output) with their stream positions t0 + t[i], t[i] < t_span;
 * device pointers */
int yakamd_feed_hashed_dev(yak_ch_t *h, const void *d_hash_u64, const void *d_t_u32, int64_t n,
                           uint64_t t0, uint64_t t_span);
/* returns the number of keys added to the table by this pass (-1 on error).  Like
 * yak_ch_insert_list it does not touch h->tot: the caller adds (count.c:138) */
int64_t yakamd_pass_end(yak_ch_t *h);

/* extraction only (count.c:28-43): hashed canonical k-mers, and their positions, of a
 * device-resident base image, restricted to prefixes [prefix_lo, prefix_hi) of a 1<<pre split --
 * one call per destination GPU gives the send buffers of the prefix exchange.  Outputs must hold
 * n_bytes entries; returns the count or -1. */
int64_t yakamd_extract_dev(int k, const void *d_bases, int64_t n_bytes,
                           void *d_hash_u64_out, void *d_t_u32_out,
                           int pre, int prefix_lo, int prefix_hi, void *stream);

/* Sharded exchange without re-extraction.  yakamd_partition_dev() turns a device-resident base
 * image into 16-byte records {yak_hash64, position} grouped by sub-table prefix (ascending), and
 * returns the 1<<pre + 1 group offsets in h_bstart; prefixes owned by one rank are contiguous, so a
 * rank's send buffer per destination is a slice.  The receiver hands every source's slice to
 * yakamd_feed_partitioned_dev() together with that slice's own offsets (h_bstart[p] = first record
 * of prefix p inside d_rec, entries outside the shard equal their neighbours).  n_bytes = 0 (no chunk)
 * returns 0 with every offset 0 and launches nothing; the same holds for the tagged and the bare-hash partition. */
int64_t yakamd_partition_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_rec_out, uint64_t *h_bstart);
int yakamd_feed_partitioned_dev(yak_ch_t *h, const void *d_rec, int64_t n, const uint64_t *h_bstart,
                                uint64_t t0, uint64_t t_span);
/* same, but d_rec is LENT: the caller keeps it valid and unmodified until yakamd_pass_end() returns,
 * and the engine works on it in place instead of taking a copy */
int yakamd_feed_partitioned_lent_dev(yak_ch_t *h, const void *d_rec, int64_t n, const uint64_t *h_bstart,
                                     uint64_t t0, uint64_t t_span);
/* The same exchange at 8 bytes per k-mer instance: TAGGED records (hash >> pre) << 12 | toggle << 10 | position in the
 * 1024-position round -- the stream order of a prefix's records is implied by the order the (round-stable) partition
 * wrote them in, so no position travels.  yakamd_tagged_ok(k, pre) != 0 iff the format applies (k < 32,
 * 2k - pre <= 52, pre <= 10); the slice of a source must arrive whole and unpermuted.  lent != 0 as above */
int yakamd_tagged_ok(int k, int pre);
int yakamd_pass_fast(yak_ch_t *h);        /* 1 while h's open pass can take tagged records (it runs on the exclusive-ownership path) */
int64_t yakamd_partition_tagged_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_rec8_out, uint64_t *h_bstart);
int yakamd_feed_partitioned_tagged_dev(yak_ch_t *h, const void *d_rec8, int64_t n, const uint64_t *h_bstart,
                                       uint64_t t0, uint64_t t_span, int lent);

/* The same for passes that only count existing keys (create_new = 0; main.c:57): 8-byte records,
 * just the yak_hash64 values, grouped by prefix the same way. */
int64_t yakamd_partition_hashes_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_hash_out, uint64_t *h_bstart);
int yakamd_count_partitioned_dev(yak_ch_t *h, const void *d_hash_u64, int64_t n, const uint64_t *h_bstart);

/* create_new = 0 pass on bare yak_hash64 values (any order): count the ones present in the table */
int yakamd_count_hashes_dev(yak_ch_t *h, const void *d_hash_u64, int64_t n);

/* The second pass of the filtered protocol reads the SAME input as the first (reference main.c:53-57: `yak count -b`
 * with one file).  yakamd_retain_input(h, 1) before the create_new = 1 pass keeps that pass's hashed, prefix-grouped
 * k-mers (8-byte tagged records) in device memory -- all of them or, beyond an eighth of the device memory
 * (YAKAMD_RETAIN_GB), none; inside the following create_new = 0 pass yakamd_count_retained(h) counts them instead of
 * a feed: 0 = every instance counted (nothing else must be fed), 1 = nothing usable was kept: feed the input as
 * usual, < 0 = error.  The records are released by the count, by the end of any count pass, by the next create_new
 * pass and by yakamd_retain_input(h, 0).  The caller vouches that both passes see the same input; yak_count() does it
 * by itself when the second call names the file of the first (same device, inode, size and modification time). */
int yakamd_retain_input(yak_ch_t *h, int on);
int yakamd_count_retained(yak_ch_t *h);
int64_t yakamd_retained_instances(yak_ch_t *h);

/* Lookup-only path (`yak qv`, reference qv.c:34-86, k < 32).  yakamd_lookup_dev(): d_out_u16[i] =
 * max(0, yak_ch_get()) of the canonical k-mer ENDING at byte i of the base image, 0xffff where no
 * k-mer ends (window shorter than k or holding a non-ACGT byte); not inside an open pass, not on a table
 * sharded over prefix ranges.  yakamd_qv_reduce_dev(): sequence j
 * is bytes [d_seq_off[j], d_seq_off[j] + d_seq_len[j]) of that image; d_tot / d_non0 receive its
 * number of k-mers / of k-mers present in the table (d_tot = 0xffffffff for a sequence shorter than
 * min_len), and every sequence with non0 >= tot * min_frac adds its values to d_hist1024 (uint64
 * bins, accumulated: zero them first). */
int yakamd_lookup_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, void *d_out_u16);
int yakamd_qv_reduce_dev(yak_ch_t *h, const void *d_t_u16, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                         int min_len, double min_frac, uint32_t *d_tot, uint32_t *d_non0, uint64_t *d_hist1024);

/* Lookup-only path of `yak triobin` (reference triobin.c:41-101, k in [1, 63]) on a table loaded with yak_ch_restore_core(...,
 * YAK_LOAD_TRIOBIN1, ...) and then (..., YAK_LOAD_TRIOBIN2, ...).  yakamd_triobin_lookup_dev(): d_flag_u8[i] = max(0, yak_ch_get())
 * of the canonical k-mer ENDING at byte i of the base image -- the flag pat class | mat class << 2 --, 0xff where no k-mer ends;
 * fails with a message (and no flag trusted) if a probed count field exceeds 15, i.e. the table was not made by those loads.  It serves
 * the three YAK_LOAD_SEXCHR1 / 2 / 3 loads of `yak sexchr` too, whose flags (1 | 2 | 4) are at most 7.  Not
 * inside an open pass, not on a table sharded over prefix ranges.  yakamd_triobin_reduce_dev(): sequence j = bytes
 * [d_seq_off[j], d_seq_off[j] + d_seq_len[j]) of that flag array; d_cnt_i32x19[19 j ..] receives c[16] (histogram of the flags of
 * its k-mers), sc[2] (the paternal / maternal solid-run sums of triobin.c:94-100) and nk (its number of k-mers).  `stream` = a
 * hipStream_t or 0; both calls return when the device is done. */
int yakamd_triobin_lookup_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, void *d_flag_u8);
int yakamd_triobin_reduce_dev(int k, const void *d_flag_u8, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                              int32_t *d_cnt_i32x19, void *stream);
/* `yak triobin` as a library call: every read of `fn` (FASTA/FASTQ, .gz, "-" = stdin) classified against `ch` (the two TRIOBIN loads),
 * output byte-equal to the reference's with -t1 (per chunk of chunk_size bases: the D lines of print_diff, then one line per read)
 * written to out_fn (NULL = stdout).  0 on success, -1 after a message on stderr. */
typedef struct {
	double ratio_thres;       /* -r, 0.33 */
	int print_diff;           /* -p, 0 */
	int n_threads;            /* -t, 8: the reference's worker threads; here the reads are looked up on the device and a second thread reads ahead */
	int64_t chunk_size;       /* bases per chunk, 200000000 (triobin.c:13) */
} yakamd_tbopt_t;
void yakamd_tbopt_init(yakamd_tbopt_t *opt);
int yakamd_triobin(const yakamd_tbopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn);

/* Streak reduction of `yak trioeval` (reference trioeval.c:89-116, k in [1, 63]) over the flags yakamd_triobin_lookup_dev() wrote:
 * a position's type is 1 where its flag is 2, 2 where it is 8, 0 elsewhere; a streak is a maximal run [st, en) of one type > 0 with
 * en - st >= min_n.  The array is bytes [0, n_bytes) of d_flag_u8; sequence j starts at d_seq_off[j] (ascending), and the byte after every
 * sequence must not be 2 or 8 (an image's '\n' is 0xff), so that no run crosses two sequences.  d_cnt_i32x6[6 j ..] receives d[0], d[1],
 * c[0..3] of sequence j (trioeval.c:92-99, int32).  With d_streaks != NULL, *d_streaks receives a device buffer (the caller frees it
 * with yakamd_dev_free; NULL when there is no streak) of *n_streaks yakamd_streak_t in sequence and position order, st and en relative
 * to the sequence.  `stream` = a hipStream_t or 0; returns when the device is done. */
typedef struct {
	uint32_t seq, st, en, type;
} yakamd_streak_t;
int yakamd_trioeval_reduce_dev(int k, int min_n, const void *d_flag_u8, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                               int64_t n_bytes, int32_t *d_cnt_i32x6, void **d_streaks, int64_t *n_streaks, void *stream);
/* `yak trioeval` as a library call: the phasing of every sequence of `fn` (FASTA/FASTQ, .gz, "-" = stdin) against `ch` (the two
 * TRIOBIN loads), output byte-equal to the reference's with -t1 (the C header; per chunk of chunk_size bases the F / E lines, then
 * one S line per sequence; then the W, H and N lines) written to out_fn (NULL = stdout).  0 on success, -1 after a message on stderr. */
typedef struct {
	int min_n;                /* -n, 2: the shortest streak */
	int print_err;            /* -e, 0: E lines at the switches */
	int print_frag;           /* 1 (-F sets 0): F lines of the fragments */
	int n_threads;            /* -t, 8: the reference's worker threads; here the sequences are reduced on the device and a second thread reads ahead */
	int64_t chunk_size;       /* bases per chunk, 1000000000 (trioeval.c:12) */
} yakamd_teopt_t;
void yakamd_teopt_init(yakamd_teopt_t *opt);
int yakamd_trioeval(const yakamd_teopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn);

/* `yak chkerr` (reference chkerr.c) on the device, k in [1, 63], on a YAK_LOAD_ALL table (yak_ch_restore).  yakamd_chkerr_lookup_dev() writes
 * one byte per position of a base image as yakamd_lookup_dev() takes it: 1 where the k-mer ending there is low, i.e. the signed
 * yak_ch_get() < min_cnt (-1 for an absent k-mer: min_cnt 0 marks the absent ones alone), 0 where it is not, 0xff where no k-mer ends.  Refused:
 * a table sharded over prefix ranges or spread over several devices, an open pass.  Returns when the device is done.
 * yakamd_chkerr_streaks_dev() finds the streaks in those bytes: maximal runs [st, en) of 1 with en - st > min_streak (every run when
 * min_streak < 0), sequence j starting at d_seq_off[j] (ascending; the byte after every sequence must not be 1, as an image's '\n' is 0xff).
 * *d_streaks receives a device buffer (free it with yakamd_dev_free; NULL when there is no streak) of *n_streaks yakamd_streak_t in sequence and
 * position order, st and en relative to the sequence, type 1; with d_streaks NULL only the number.  `stream` = a hipStream_t or 0. */
int yakamd_chkerr_lookup_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, int min_cnt, void *d_low_u8);
int yakamd_chkerr_streaks_dev(int min_streak, const void *d_low_u8, const uint64_t *d_seq_off, int64_t n_seq, int64_t n_bytes,
                              void **d_streaks, int64_t *n_streaks, void *stream);
/* `yak chkerr` as a library call: the streaks of low k-mers of every sequence of `fn` (FASTA/FASTQ, .gz, "-" = stdin) in `ch`, printed as the
 * reference prints them with -t1 (`name \t start \t end \t length` per streak, input order; with min_streak < 0 also its line `name \t 1-k \t 0 \t 0`
 * ahead of each sequence's streaks) to out_fn (NULL = stdout).  0 on success, -1 after a message on stderr. */
typedef struct {
	int min_cnt;              /* -c, 3: a k-mer is low when its count is below this (-1 when absent) */
	int min_streak;           /* -s, 5: a streak is printed when longer than this */
	int n_threads;            /* -t, 8: the reference's worker threads; here the sequences are looked up on the device and a second thread reads ahead */
	int64_t chunk_size;       /* bases per chunk, 1000000000 (chkerr.c:103) */
} yakamd_ceopt_t;
void yakamd_ceopt_init(yakamd_ceopt_t *opt);
int yakamd_chkerr(const yakamd_ceopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn);

/* `yak sexchr` (reference sexchr.c) on the device.  The table is the three loads yak_ch_restore_core(0, chrY, YAK_LOAD_SEXCHR1), (ch, chrX,
 * YAK_LOAD_SEXCHR2), (ch, PAR, YAK_LOAD_SEXCHR3); yakamd_triobin_lookup_dev() looks a chunk up in it (flags 0-7).  yakamd_sexchr_reduce_dev()
 * tallies those flags per sequence: d_cnt_u64x4[4 j ..] = n_k (positions of sequence j where a k-mer ends), n_sexchr (flag > 0), n_sex1 (flag == 1),
 * n_sex2 (flag == 2), overwritten; sequence j is bytes [d_seq_off[j], d_seq_off[j] + d_seq_len[j]) (ascending) of the n_bytes of d_flag_u8.
 * `stream` = a hipStream_t or 0; returns when the device is done. */
int yakamd_sexchr_reduce_dev(const void *d_flag_u8, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq, int64_t n_bytes,
                             uint64_t *d_cnt_u64x4, void *stream);
/* `yak sexchr` as a library call: the two header lines, then one S line per sequence of fn_hap1 (hap 1), then of fn_hap2 (hap 2), in input order,
 * byte-equal to the reference's -t1 output, to out_fn (NULL = stdout).  0 on success, -1 after a message on stderr. */
typedef struct {
	int n_threads;            /* -t, 8: as yakamd_ceopt_t's */
	int64_t chunk_size;       /* -K, bases per chunk, 1000000000 (sexchr.c:13) */
} yakamd_scopt_t;
void yakamd_scopt_init(yakamd_scopt_t *opt);
int yakamd_sexchr(const yakamd_scopt_t *opt, const yak_ch_t *ch, const char *fn_hap1, const char *fn_hap2, const char *out_fn);

/* `yak print` (reference main.c:286-323) on the device: the stored k-mers of sub-tables [sub_lo, sub_hi), sub-table after sub-table in ascending
 * slot order -- what yak_ch_getseq() returns for each of them, without a host mirror of the table.  k must be below 32 (htab.c:359); the table is
 * listed as it is (yak_ch_tighten() first for the reference's order).  A table sharded over prefix ranges is served when its shards are on one
 * device (yakamd_print: on any), not inside an open pass.
 * yakamd_kmers_dev(): k-mer i as d_x_u64[i] (2 bits per base, the first base highest) and its count as d_c_u16[i], caller-owned device arrays of
 * `cap` elements.  Returns the number of k-mers; when cap is smaller or a pointer is NULL, the number needed, and nothing is written.
 * yakamd_print_dev(): the bytes main.c:308-317 writes for them -- k letters and '\n', or with_counts letters, '\t', the count in decimal and '\n' --
 * into d_text (cap_bytes); the same convention for the byte count.  -1 after a message (yakamd_last_error()). */
int64_t yakamd_kmers_dev(yak_ch_t *h, int sub_lo, int sub_hi, void *d_x_u64, void *d_c_u16, int64_t cap);
int64_t yakamd_print_dev(yak_ch_t *h, int sub_lo, int sub_hi, int with_counts, void *d_text, int64_t cap_bytes);
/* the whole table as text to out_fn (NULL or "-" = stdout; a pipe works), in ranges of whole sub-tables whose text fits batch_bytes of device
 * memory (two such buffers are held) -- a sub-table is never split, so the largest sub-table's text is the floor of a range whatever
 * batch_bytes says.  The text crosses the bus in pinned pieces and is written while the next range is formatted.  0, or -1 after a message
 * (k >= 32: before anything is written) */
typedef struct {
	int32_t with_counts;      /* -c, 0: a tab and the count behind every k-mer */
	int32_t n_threads;        /* 4: accepted for symmetry with the other commands; one thread copies and writes */
	int64_t batch_bytes;      /* device bytes of one range's text, 256 MiB */
} yakamd_propt_t;
void yakamd_propt_init(yakamd_propt_t *opt);
int yakamd_print(const yakamd_propt_t *opt, const yak_ch_t *ch, const char *out_fn);
/* how often this process has copied a table image to its host mirror (yakamd_sync_host and the yak.h calls that read the mirror: yak_ch_get,
 * yak_ch_getseq); the listing above never does */
int64_t yakamd_host_syncs(void);

/* `yak inspect` (reference inspect.c) on the device.  yakamd_inspect_dev() is its join: every stored key of table A adds one to
 * d_joint[c0 * 1024 + c1] (uint64 bins, accumulated: zero them first), c0 = key & 1023 its count in A, c1 = max(0, yak_ch_get(b, h)) its count in
 * b (0 when b is NULL: one table).  The keys are those of A's sub-tables [sub_lo, sub_hi) in dump order, d_sub_off[j] = keys before sub-table
 * sub_lo + j (sub_hi - sub_lo + 1 device words, the last = n_keys); headers != 0: d_keys is the .yak body itself, each sub-table's 8-byte
 * {capacity, size} word in front of its keys.  The probe hash h is (key >> 10) << pre_a | i for a key of sub-table i -- the k-mer's hash (all of
 * it at k < 32; at k >= 32 its bits [0, pre + 54), so the two tables must have the same pre there) --, or with ref_probe the stored key itself,
 * as inspect.c:58 passes it.  b may be sharded over prefix ranges of one device; not a table spread over several devices, not inside an open
 * pass; its k must be k.  `stream` = a hipStream_t or 0; returns when the device is done. */
int yakamd_inspect_dev(yak_ch_t *b, int k, int pre_a, int sub_lo, int sub_hi, const void *d_keys, int64_t n_keys,
                       const uint64_t *d_sub_off, int headers, int ref_probe, uint64_t *d_joint, void *stream);
/* `yak inspect` as a library call: the HS lines of in1 (fn2 NULL), or its SN and QV lines against fn2, printed as inspect.c prints them to
 * out_fn (NULL = stdout); with ref_probe and two tables byte-equal to the reference's.  in1 is streamed in batches of about batch_keys keys.
 * 0 on success, -1 after a message on stderr (and nothing written) */
typedef struct {
	int max_cnt;              /* -m, 20: the SN columns and QV lines, in [0, 1023] */
	int ref_probe;            /* -R, 0: probe in2 with the stored key as inspect.c:58 does (finds few of the shared k-mers) */
	int n_threads;            /* -t, 4: yak_ch_hist's threads; in1 is read ahead on a second thread */
	int64_t batch_keys;       /* keys of in1 per device batch, 1 << 24 */
} yakamd_inopt_t;
void yakamd_inopt_init(yakamd_inopt_t *opt);
int yakamd_inspect(const yakamd_inopt_t *opt, const char *fn1, const char *fn2, const char *out_fn);
/* the same join on two resident tables (b NULL: one), such as yak_count()'s: joint = 1024 x 1024 int64 host bins, overwritten.  Either table
 * may be sharded over prefix ranges of one device; both on the same device.  0, or -1 after a message */
int yakamd_inspect_tables(const yak_ch_t *a, const yak_ch_t *b, int ref_probe, int64_t *joint);

/* Add the counts of two tables (not in the reference: yak_ch_merge is cntasm's presence merge, which adds ONE per k-mer of h1 whatever its count).
 * Afterwards h0 holds every k-mer that was in h0, or in h1 with a count of at least 1, at min(1023, count in h0 + count in h1), a k-mer absent
 * from a table counting 0 there; h0->tot = the number of stored keys.  h1 is only read and is NOT consumed; its keys of count 0 contribute
 * nothing and do not enter h0.  The sum is exact for unfiltered tables (`yak count -b0`: the table of lane 1 plus the table of lane 2 is the table
 * of both); two bloom-filtered tables are summed as they are -- what their filters and the shrink to counts >= 2 dropped stays dropped.
 * Layout: h0 gets exactly the slots yak_ch_merge(h0, h1', 1, 1023, n_thread, pre_resize) gives it, h1' a throw-away copy of h1 -- the put-calls
 * are h1's keys of count >= 1, sub-table by sub-table in h1's slot order, khashl growing at the next put-call after 75 % load, the optional
 * pre-resize (htab.c:262-266) included -- and only the count fields differ from what that merge stores; the .yak bytes are a function of the two
 * operands.  On the device: that merge's create pass, then one probe per listed key that rewrites its count field; no host mirror is read.
 * k in [1, 63] (the stored key holds hash bits [pre, pre + 54), which the listing hands back unchanged).  Either table may be sharded over prefix
 * ranges; operands on different devices take yak_ch_merge's routes (peer access, or a staged copy).  0, or -1 after a message
 * (yakamd_last_error()) -- NULL or not an engine table, the same table twice, different k or pre, an open pass on either table: h0 is then untouched */
int yakamd_ch_sum(yak_ch_t *h0, const yak_ch_t *h1, int pre_resize);

/* Per-sequence and per-window k-mer depth (not in the reference): how often the k-mers along a sequence occur in a count
 * table.  A sequence of L bases is cut into windows of w k-mer START positions, window j covering the starts [j w, min(L, (j + 1) w)); w = 0 is one
 * window, the whole sequence; a sequence has max(1, ceil(L / w)) windows, an empty one too.  The k-mer starting at s is element s + k - 1 of the array
 * yakamd_lookup_dev() writes for the sequence, so a window is a shifted slice of it; its k-mers are the elements of that slice inside the sequence that
 * are not 0xffff (starts >= L - k + 1 have none), an absent k-mer counting 0.  Per window: n_kmer, n_present (count > 0), sum of the counts, median
 * -- the LOWER median, index (n_kmer - 1) / 2 of the sorted counts -- and max; median and max are 0 without a k-mer.  All integers, a pure function of
 * the array.
 * yakamd_depth_reduce_dev(): d_cnt_u16 = that array for a base image of n_bytes bytes (16-byte aligned, its allocation a multiple of 16 bytes; an
 * element above 1023 other than 0xffff is read as 1023), sequence j = elements [d_seq_off[j], d_seq_off[j] + d_seq_len[j]) (disjoint), d_win_off[j] =
 * the windows of the sequences before j (n_seq + 1 device words: the exclusive scan of the windows per sequence and their total); d_win receives one
 * yakamd_win_t per window, sequences in order, windows ascending.  k below 32.  It needs no table.  `stream` = a hipStream_t or 0; returns when the
 * device is done. */
typedef struct { uint32_t n_kmer, n_present, median, max; uint64_t sum; } yakamd_win_t;
int yakamd_depth_reduce_dev(int k, int64_t w, const void *d_cnt_u16, const uint64_t *d_seq_off, const uint32_t *d_seq_len,
                            const uint64_t *d_win_off, int64_t n_seq, int64_t n_bytes, yakamd_win_t *d_win, void *stream);
/* `yak-amd depth` as a library call: every sequence of `fn` (FASTA/FASTQ, .gz, "-" = stdin) against `ch`, a YAK_LOAD_ALL table (yak_ch_restore) or a
 * resident one, k below 32.  To out_fn (NULL = stdout): the line `#name start end n_kmer n_present mean median max` (tab-separated, as all lines), then
 * one line per window, sequences in input order, windows ascending: start and end are the window's bounds in bases, mean is "%.3f" of sum / n_kmer
 * (0.000 without a k-mer).  Per chunk of chunk_size bases the lookup, then the reduction; no host mirror of the table is built.  0 on success, -1
 * after a message on stderr -- before anything is written for k >= 32, a negative window, a table sharded over prefix ranges or spread over several
 * devices, an open pass and an input that cannot be opened. */
typedef struct {
	int64_t window;           /* -w, 0: k-mer starts per window; 0 = one window per sequence */
	int n_threads;            /* -t, 8: accepted for symmetry with the other commands; a second thread reads ahead */
	int64_t chunk_size;       /* -K, bases per chunk, 1000000000 (as yakamd_ceopt_t's) */
} yakamd_dpopt_t;
void yakamd_dpopt_init(yakamd_dpopt_t *opt);
int yakamd_depth(const yakamd_dpopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn);

/* The het-mer pairs of a count table (not in the reference): the k-mers that differ in the middle base alone, with the counts
 * of both -- the input of a Smudgeplot / PloidyPlot style ploidy analysis.  The table is a YAK_LOAD_ALL one (yak_ch_restore) or a resident one
 * (yak_count), k odd and below 32; a stored k-mer whose count is below min_cnt (in [1, 1023]) is absent, as a member and as a partner.  x = a stored
 * canonical k-mer as yakamd_kmers_dev() lists it; for d = 1, 2, 3: y' = x ^ d << (k - 1), y = min(y', revcomp_k(y')); the partners of x are the
 * distinct y != x in the table.  x and its partners are a group of 1 to 4 members, counted once; a group of two {x < y} is a pair and adds one to
 * J[min(cx, cy)][max(cx, cy)].  All of it is a pure function of the table's contents and min_cnt.
 * yakamd_hetmers_dev(): d_joint[lo * 1024 + hi] = J (1024 x 1024 uint64 device bins, accumulated: zero them first), d_group[s] += groups of s
 * members (5 uint64 device words, [0] unused).  `stream` = a hipStream_t or 0; returns when the device is done.
 * yakamd_hetmer_pairs_dev(): the pairs as records with x < y, in the table's listing order of x (sub-tables ascending, slots ascending -- the order
 * of yakamd_kmers_dev()), into d_pairs (cap records, device memory).  Returns their number = the sum of J; when cap is smaller or d_pairs is NULL,
 * the number needed, and nothing is written.
 * Both stage the table's keys in ranges of whole sub-tables of at most 2^24 keys and probe the whole resident table; neither builds a host mirror.
 * -1 after a message (yakamd_last_error()), before any device work: NULL or not an engine table, an even k, k >= 32, min_cnt outside [1, 1023], an
 * open pass, a table sharded over prefix ranges or spread over several devices, no gfx950 GPU. */
typedef struct { uint64_t x, y; uint32_t cx, cy; } yakamd_hetpair_t;   /* x < y */
int yakamd_hetmers_dev(yak_ch_t *h, int min_cnt, uint64_t *d_joint, uint64_t *d_group, void *stream);
int64_t yakamd_hetmer_pairs_dev(yak_ch_t *h, int min_cnt, void *d_pairs, int64_t cap);
/* `yak-amd hetmers` as a library call.  To out_fn (NULL or "-" = stdout), tab-separated: the line `#hetmers k=<k> min_cnt=<min_cnt>`; with
 * print_pairs one line `K <k-mer x> <cx> <k-mer y> <cy>` per pair in listing order (letters as yak print writes them), produced range by range;
 * `G <s> <groups of s members>` for s = 1 .. 4; `P <lo> <hi> <J[lo][hi]>` for every non-zero bin, lo ascending, then hi.  0 on success; -1 after
 * a message on stderr -- on one of the refusals above before the output is created. */
typedef struct {
	int32_t min_cnt;          /* -c, 1: a k-mer below this count is absent */
	int32_t print_pairs;      /* -p, 0: the K lines */
	int64_t batch_keys;       /* keys staged per range of whole sub-tables, 2^24 */
} yakamd_hmopt_t;
void yakamd_hmopt_init(yakamd_hmopt_t *opt);
int yakamd_hetmers(const yakamd_hmopt_t *opt, const yak_ch_t *ch, const char *out_fn);

/* The de Bruijn graph of a count table (not in the reference): the graph its k-mers span, its compacted form and its unitigs --
 * what BCALM2, Cuttlefish or the first stage of ABySS build from a table of their own.  The table is a YAK_LOAD_ALL one or a resident one, k odd and
 * below 32, min_cnt in [1, 1023]; everything is a pure function of the table's {(k-mer, count)} and of min_cnt.
 * A NODE is a stored canonical k-mer x, coded as yakamd_kmers_dev() lists it, with a count of at least min_cnt; a stored key below it is absent, as
 * a node and as a neighbour.  The LISTING INDEX of a stored key is its place in yakamd_kmers_dev(h, 0, 1 << pre, ...); a key that is no node keeps
 * its index.  Side 0 (R) appends a base b: z = (x << 2 | b) & (4^k - 1); side 1 (L) prepends it: z = x >> 2 | b << 2 (k - 1); the neighbour is
 * y = min(z, revcomp_k(z)).  `edges` has bit b set iff the R extension by b is a node, bit 4 + b iff the L extension is (y may be x itself); the
 * degree of a side is the popcount of its four bits.  y faces x with side t: from R, t = L if y == z, else R; from L, t = R if y == z, else L.  Side
 * (x, s) is LINKED to (y, t) iff it has one edge, y != x and (y, t) has one edge; links are symmetric.  A UNITIG is a maximal chain of linked nodes:
 * open with two unlinked end sides (a node without a link is one), or a cycle; open unitigs = n_node - n_linked_side / 2.
 * yakamd_graph_open() probes the table for every node's eight possible neighbours once and keeps about 1.125 bytes of device memory per slot of the
 * table and 16 per sub-table until yakamd_graph_close(); the caller leaves the table unchanged in between.  NULL after a message
 * (yakamd_last_error()), before any device work: NULL or not an engine table, an even k, k >= 32, min_cnt outside [1, 1023], an open pass (refused
 * again at each later call), a table sharded over prefix ranges or spread over several devices, no gfx950 GPU.  A table marked as
 * homopolymer-compressed is taken as it is.
 * yakamd_graph_stats(): the tallies; deg[l][r] = nodes of l left and r right edges, n_arc = the sum of all degrees.  0, or -1 after a message.
 * yakamd_graph_nodes_dev(): one record per stored key of sub-tables [sub_lo, sub_hi) in listing order into d_nodes (cap records of 32 bytes, device
 * memory, 16-byte aligned), aligned with yakamd_kmers_dev() of the same range: x and count are its output; link[s] = the GLOBAL listing index of the
 * node side s is linked to << 1 | the side of it that faces back, or YAKAMD_GRAPH_NONE; a key that is no node has edges = 0 and no link.  Returns the
 * number of records; with a smaller cap or a NULL pointer the number needed, and nothing is written.  -1 after a message.
 * No call builds a host mirror of the table. */
typedef struct yakamd_graph yakamd_graph_t;
#define YAKAMD_GRAPH_NONE (~(uint64_t)0)
typedef struct { uint64_t n_key, n_node, n_arc, n_linked_side, deg[5][5]; } yakamd_gstat_t;
typedef struct { uint64_t x, link[2]; uint32_t count, edges; } yakamd_gnode_t;
yakamd_graph_t *yakamd_graph_open(yak_ch_t *h, int min_cnt);
int     yakamd_graph_stats(yakamd_graph_t *g, yakamd_gstat_t *st);
int64_t yakamd_graph_nodes_dev(yakamd_graph_t *g, int sub_lo, int sub_hi, void *d_nodes, int64_t cap);
void    yakamd_graph_close(yakamd_graph_t *g);
void    yakamd_graph_open_ms(yakamd_graph_t *g, double ms[3]);   /* measurement: the milliseconds of the open's edge, rank and link steps, taken only with YAKAMD_VERBOSE or the test switch YAKAMD_GRAPH_TIMED */
/* `yak-amd unitigs` as a library call: the graph, its records pulled to the host in ranges of whole sub-tables of at most batch_keys keys, and the
 * walk along the links there with n_threads threads (32 bytes of host memory per stored key; a table whose records do not fit fails with a message
 * that says so).  Open unitigs come first, ascending by the listing index of their start node -- the end node with the smaller index, read away
 * from its unlinked side; a node without a link as stored -- then the cycles, ascending by their smallest index, from that node as stored through
 * R.  Reading a node "as stored" leaves it through R, reading its reverse complement through L.  A unitig of n nodes has n + k - 1 bases.
 * To out_fn (NULL or "-" = stdout) as FASTA: `>u<j>\tLN:i:<bases>\tKC:i:<sum of its nodes' counts>\tkm:f:<KC / nodes, %.1f>\tCL:i:<1 for a cycle,
 * else 0>` and the bases on one line, j from 0.  With stats_only, tab-separated instead: `#unitigs k=<k> min_cnt=<c>`; `N n_key n_node n_arc
 * n_linked_side`; `D l r deg[l][r]` per non-zero bin, l ascending, then r; `U n_open n_cycle sum_len max_len n50` in bases, n50 = the largest L such
 * that the unitigs of at least L bases hold half of sum_len or more (0 without a node).  0 on success; -1 after a message on stderr -- on one of the
 * refusals above before the output is created. */
typedef struct {
	int32_t min_cnt;          /* -c, 1: a k-mer below this count is absent */
	int32_t stats_only;       /* -s, 0: the N, D and U lines, not the FASTA */
	int32_t n_threads;        /* -t, 8: threads of the host walk */
	int64_t batch_keys;       /* keys per range of whole sub-tables pulled to the host, 2^24 */
} yakamd_ugopt_t;
void yakamd_ugopt_init(yakamd_ugopt_t *o);
int  yakamd_unitigs(const yakamd_ugopt_t *o, const yak_ch_t *ch, const char *out_fn);
void yakamd_unitigs_ms(double ms[4]);   /* measurement: the milliseconds the process' last yakamd_unitigs call spent on the graph, the records' way to the host, the host walk, the text */

/* Homopolymer compression (HPC; not in the reference): every run of the same base collapses to one base before k-mers are taken,
 * the space long-read assemblers and their QV pipelines count in.  On a base image as described at the top of this file: a position is VALID when its
 * byte has a code 0..3 under seq_nt4_table (in the packed form: its validity bit).  Position i is DROPPED iff i > 0, i and i - 1 are both valid and
 * their codes are equal; every other position is KEPT, an invalid one too, so an invalid position ends the run before it (AANAA -> ANA; Aa and TU are
 * one base each).  The output is the kept positions in order as an ASCII image -- 'A' 'C' 'G' 'T' for a valid one, '\n' for an invalid one -- and '\n'
 * from n_out up to the next multiple of 16: what compressing every record's sequence on the host and building the image from the result gives.
 * yakamd_hpc_dev(): the ASCII image; with n_seq > 0 also, for sequence j = bytes [d_seq_off[j], d_seq_off[j] + d_seq_len[j]) of the input,
 * d_seq_off_out[j] = kept positions before d_seq_off[j] and d_seq_len_out[j] = kept positions inside it (the arrays may be NULL with n_seq 0).
 * yakamd_hpc_packed_dev(): the packed image of yakamd_feed_packed_dev().  Inputs 16-byte aligned (d_valid: 4); d_out 16-byte aligned, not overlapping
 * the input, with room for n rounded up to 16.  Both return n_out (0 for an empty image, without a launch) or -1 after a message, need no table and
 * return when the device is done; `stream` = a hipStream_t or 0.  yakamd_hpc_host(): the same function in plain C++ on host memory, no device. */
int64_t yakamd_hpc_dev(const void *d_bases, int64_t n_bytes, void *d_out, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                       uint64_t *d_seq_off_out, uint32_t *d_seq_len_out, void *stream);
int64_t yakamd_hpc_packed_dev(const void *d_codes, const void *d_valid, int64_t n_bases, void *d_out, void *stream);
int64_t yakamd_hpc_host(const void *ascii, int64_t n_bytes, void *out);
/* Tables that live in HPC space.  The .yak format cannot record the space and yak_copt_t is the reference's: the mark is on the table (dump and restore
 * do not carry it: mark a restored table again).  While a table is marked, every feed of BASES into it -- yakamd_feed_bases_*, yakamd_feed_packed_*,
 * every reader route of yak_count() and the chunks of a multi-GPU job -- is compacted on the device first; t0 stays the uncompressed stream position of
 * the feed.  Feeds of hashes or partitioned records are taken as they are: their producer chose the space.  yak_qv() on a marked table compacts every
 * chunk before it looks it up, and min_len, the SQ lengths and the EK positions are in compressed coordinates; yakamd_triobin, yakamd_trioeval,
 * yakamd_chkerr, yakamd_sexchr and yakamd_depth refuse a marked table with a message before any output.  Table-to-table calls ignore the mark.
 * yakamd_ch_set_hpc(): 0, or -1 after a message inside an open pass; a table sharded over ranks has every shard marked.
 * yakamd_count_hpc(): yak_count() in HPC space -- h0 == 0: the new table is marked before its first feed; h0 marked: its k-mers are counted
 * (yak_count(fn, opt, h0) does the same: the mark governs, so the filtered two-pass protocol works with either call); h0 unmarked: refused, NULL.
 * A sequence longer than a multi-GPU chunk is cut so that the next chunk opens with the last k - 1 KEPT positions of the one before. */
int yakamd_ch_set_hpc(yak_ch_t *h, int on);
int yakamd_ch_hpc(const yak_ch_t *h);
yak_ch_t *yakamd_count_hpc(const char *fn, const yak_copt_t *opt, yak_ch_t *h0);

/* Which bases of a sequence lie inside k-mers that a table holds, lacks or holds too often (not in the reference).  t = the
 * array yakamd_lookup_dev() writes for a base image of n_bytes bytes, k below 32, and a predicate [lo, hi] with 0 <= lo <= hi <= 1023:
 *   hit(j)  = t[j] != 0xffff and lo <= min(t[j], 1023) <= hi (an absent k-mer reads 0, so 0:0 selects "the table lacks it")
 *   cov(i)  = 1 if some j in [i, min(i + k - 1, n_bytes - 1)] has hit(j), else 0: base i lies inside at least one hitting k-mer
 * over the flat array; on a real image no cover crosses a record and an invalid byte is never covered, because the k-mer ending at j contains every
 * byte back to i.  Per sequence s = elements [off[s], off[s] + len[s]): n_kmer = elements that are not 0xffff, n_hit = elements with hit, n_cov =
 * the sum of cov, n_run = positions with cov(i) = 1 and (i == off[s] or cov(i - 1) == 0).  The masked image m: soft, m[i] = b[i] | 0x20 where cov(i)
 * and b[i] is an ASCII letter, else b[i] (raw bytes 0..3 stay); hard, m[i] = 'N' where cov(i), else b[i].
 * yakamd_cover_dev(): one pass (kern_cover.inc).  d_cov_u8 receives cov, one byte per position -- what yakamd_chkerr_streaks_dev(-1, ...) takes to
 * list the covered intervals per sequence -- and with mask 1 (soft) or 2 (hard) d_masked the masked image of d_bases; both are written up to the
 * next multiple of 16 (0 and '\n' from n_bytes on) and not behind it.  d_tally[0 .. n_seq) is overwritten (it may be NULL with n_seq = 0); d_bases and
 * d_masked may be NULL with mask 0.  The count, cover and image arrays are 16-byte aligned with room for n_bytes rounded up to 16 elements; the
 * sequences ascend and are disjoint.  It needs no table.  `stream` = a hipStream_t or 0; returns when the device is done; n_bytes = 0 launches
 * nothing.  -1 after yakamd_last_error() is set, before any device work: k outside [1, 31], lo / hi outside 0 <= lo <= hi <= 1023, mask outside
 * 0..2, mask != 0 with a NULL image, a misaligned array, a negative size. */
typedef struct { uint32_t n_kmer, n_hit, n_cov, n_run; } yakamd_cov_t;
int yakamd_cover_dev(int k, int lo, int hi, const void *d_cnt_u16, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                     const void *d_bases, int mask, void *d_cov_u8, void *d_masked, yakamd_cov_t *d_tally, void *stream);
/* `yak-amd cover` as a library call: every sequence of `fn` (FASTA/FASTQ, .gz, "-" = stdin) against `ch`, a YAK_LOAD_ALL table (yak_ch_restore) or a
 * resident one, k below 32.  Per chunk of chunk_size bases the lookup, then yakamd_cover_dev, with intervals the run finder of chkerr on the cover
 * bytes; the host gets tallies and intervals, never the cover bytes, and the masked image in FASTA mode alone.  A sequence is selected iff
 * (n_hit >= min_hit && (double)n_cov >= min_frac * (double)len) != invert.  To out_fn (NULL = stdout), tab-separated:
 *   mask < 0   `#cover k=<k> lo=<lo> hi=<hi>`; per selected sequence in input order `S name len n_kmer n_hit n_cov n_run` and, with intervals,
 *              directly behind it its `B name start end` lines (0-based, half-open, in bases, ascending); last `T n_seq n_selected sum_len
 *              sum_kmer sum_hit sum_cov`, the sums over all sequences, selected or not
 *   mask >= 0  `>name`, then the sequence's bytes of the masked image (of the image itself with mask 0), per selected sequence and nothing else; the
 *              chunk reader carries neither qualities nor header comments
 * Sequences are never cut by a chunk, so the output does not depend on chunk_size.  0 on success, -1 after a message on stderr -- before the output
 * is created for k >= 32, a table sharded over prefix ranges or spread over several devices, a table marked as homopolymer-compressed, an open
 * pass, an input that cannot be opened, lo / hi outside 0 <= lo <= hi <= 1023, mask above 2, min_frac outside [0, 1] and a negative min_hit. */
typedef struct {
	int32_t lo, hi;           /* -c LO[:HI], 1:1023; -c N = N:1023 */
	int32_t intervals;        /* -b, 0: B lines */
	int32_t mask;             /* -m none|soft|hard (0, 1, 2): FASTA out instead of the table; -1 = table (default) */
	int32_t invert;           /* -v, 0 */
	int64_t min_hit;          /* -n, 0 */
	double  min_frac;         /* -f, 0.0 */
	int     n_threads;        /* -t, 8: accepted as in the other commands */
	int64_t chunk_size;       /* -K, 1000000000 */
} yakamd_cvopt_t;
void yakamd_cvopt_init(yakamd_cvopt_t *opt);
int yakamd_cover(const yakamd_cvopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn);

/* Host-only test hook (no device needed): the base image yak_count() hands to the device for a
 * FASTA/FASTQ(.gz) file -- sequences of >= min_len bases, each followed by '\n'.  use_fast_path = 0
 * forces the general record reader for every record.  *out is malloc()ed; returns its length or -1. */
int64_t yakamd_host_image(const char *fn, int min_len, int use_fast_path, char **out);
/* the same stream as yak_count() really hands it over: packed by the parser threads, one image per window -- here unpacked again, a base as
 * 'A' 'C' 'G' 'T', any other position (N, the end of a record, the positions that pad a parsed segment to a multiple of 32) as '\n'.
 * -1 if the file is not one the parallel parser takes (a pipe, a file read by one thread). */
int64_t yakamd_host_image_packed(const char *fn, int min_len, char **out);
/* Host-only test hooks of the reader for ordinary gzip files (csrc/pgz.h; replaces gzread() behind kseq.h:80-96 for yak_count()):
 * the compressed bytes one thread takes per batch, the smallest file the reader takes and the room it keeps in front of a batch for the
 * record the parser carries over (0 / negative: unchanged; defaults 1 MiB, 4 MiB, 64 MiB);
 * the inflated stream of `fn` (malloc()ed *out; -1: not taken, -2: the stream is invalid -- yakamd_last_error()). */
/* Test switches: names that force a code path which the size or shape of the input would otherwise select (INTEGRATION.md section 4 lists
 * them).  No environment variable reaches them; a value set here also overrides the environment for the public knobs.  reset: forget all. */
void yakamd_test_set(const char *name, int64_t value);
void yakamd_test_reset(void);
/* The launch tally (tests/paths_util.py): one counter per kernel instantiation the library can launch, named as its launch site writes it
 * (`k_part2_wc8<false,7>`), bumped once per launch; behind them the path events (`event:...`), decisions of the host that are not launches --
 * a refused bitmap ranking, a streaming replay used or refused, sub-buckets k_lc2 passed on, slices of a pass, the path of the count pass ...
 * (`event:par_ok` / `event:par_fail` advance when yakamd_debug_counters() reads the device's counters).  Host data only: the names are known
 * once the library is loaded, no device is needed.  names: -> the number of counters, *names = their names (the library's, valid for its
 * lifetime); read: the first n counts; reset: all to zero. */
int yakamd_tally_names(const char *const **names);
void yakamd_tally_read(uint64_t *out, int n);
void yakamd_tally_reset(void);
void yakamd_gz_tune(int64_t chunk_bytes, int64_t min_file_bytes, int64_t front_bytes);
int64_t yakamd_gz_inflate(const char *fn, int n_threads, char **out);

/* device buffers for harnesses that do not bring their own allocator (tests; bench.py uses torch) */
void *yakamd_dev_alloc(size_t bytes);
void yakamd_dev_free(void *p);
int yakamd_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int yakamd_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);

/* diagnostics: [0] doublings done by the parallel replay routine, [1] sent back to the serial one */
void yakamd_debug_counters(uint32_t *out4);

/* yak_count() on several GPUs with the input already in HBM (the multi-GPU driver of reference count.c:129-143's kt_for over prefixes, without
 * the reader): the stream is cut into rounds of one chunk per DISTINCT device of dev_of_rank (in the order the devices first appear there); chunk s
 * of round b lies at d_chunk[b * S + s] on that device, n_bytes[b * S + s] bytes of the base image (ASCII, sequences separated by a non-ACGT byte;
 * at most 2^31 - 4096; 0 = none); stream order = round by round, device by device, exactly as yak_count() deals a file under YAKAMD_GPUS.  Every
 * device groups its chunk's k-mers by prefix, one RCCL grouped send / recv per round (or peer copies, or nothing on one device) moves them to their
 * owners, each rank counts its prefix range.  h0 == 0: returns a new table sharded over n_rank ranks (every yak_ch_* entry point takes it);
 * h0 != 0 (a table this call made): counts the chunks' k-mers that are in it (count.c:155-157) and returns h0.  NULL on failure.
 * *exchange_out (may be NULL): 0 nothing exchanged (one device), 1 RCCL, 2 peer copies, 3 the library's in-process test rig (test switch YAKAMD_MGPU_LOOPBACK) */
yak_ch_t *yakamd_count_multi_dev(const yak_copt_t *opt, yak_ch_t *h0, int n_rank, const int *dev_of_rank, int n_rounds,
                                 const void *const *d_chunk, const int64_t *n_bytes, int *exchange_out);

/* runtime services for callers without a HIP runtime of their own: page-locked host memory, a device-wide synchronise, free / total device memory */
void *yakamd_host_alloc(size_t bytes);
void yakamd_host_free(void *p);
int yakamd_device_sync(void);
int yakamd_mem_info(size_t *free_bytes, size_t *total_bytes);

/* high-water mark of the device memory the library had in use on device `dev` (buffers handed out by its pool; the idle ranges it keeps for the next
 * pass do not count); reset != 0 starts a new measurement from what is in use now */
int64_t yakamd_peak_bytes(int dev, int reset);
/* release the device-memory cache kept between passes (memory pool) */
void yakamd_trim(void);
/* one line per tier on stderr: what the current device's pool has obtained from the driver, holds in use and idle, and how its large buffers came about */
void yakamd_pool_report(const char *what);
/* how many ranks this process's last yak_count() ran as (> 1 on one device: the pass went in that many sweeps over prefix ranges -- YAKAMD_GPUS, or the
 * library's own rule for large unfiltered inputs, which takes more sweeps while the process does not own the device memory of fewer: INTEGRATION.md section 4) */
int yakamd_last_sweeps(void);

/* bring the host view (slot arrays reachable from yak_ch_t) up to date with HBM */
int yakamd_sync_host(yak_ch_t *h);
/* serialise the table in .yak format straight from the host view into memory (malloc'ed) */
int64_t yakamd_dump_mem(yak_ch_t *h, uint8_t **out);
/* the bytes of sub-tables [lo, hi) alone ({u32 capacity, u32 size, keys in slot order} each, htab.c:385-389; no header): one rank's share of the
 * .yak file of a prefix-sharded job; malloc'ed, returns the size or -1 */
int64_t yakamd_dump_range_mem(yak_ch_t *h, int lo, int hi, uint8_t **out);
/* k and pre of a .yak file's header: what a command compares between its tables before it loads any.  0, or -1 after a message (yakamd_last_error()):
 * the file cannot be opened, it is shorter than a header, it does not start with the magic.  No device call */
int yakamd_yak_header(const char *fn, int *k, int *pre);

/* sub-table shape, for tests: capacity and size of sub-table i (device-authoritative) */
int yakamd_subtable(yak_ch_t *h, int i, uint32_t *capacity, uint32_t *size);

/* timing / traffic counters of the last pass (filled by pass_end) */
typedef struct {
	double ms_extract, ms_insert, ms_bloom, ms_select, ms_sort, ms_replay, ms_total;
	double ms_dominant_kernel;      /* accumulated duration of the insert kernel launches */
	int64_t n_dominant_launches;
	int64_t n_instances;            /* valid k-mer windows consumed */
	int64_t n_distinct_seen;        /* distinct k-mers observed by the pass (create_new only) */
	int64_t n_new_keys;             /* keys that entered the table */
	int64_t n_bloom_candidates;     /* keys that needed exact in-batch bloom resolution */
	double ms_part2;                /* level-2 partition (part of ms_extract) */
	double ms_shrink;               /* last yak_ch_shrink on this table: compaction + layout replay */
	int64_t pass2_path;             /* how yakamd_count_retained counted this pass: 0 it did not, 1 the counts the pass before found (k_cnt2_apply
	                                 * alone), 2 a recount of the retained sub-bucket records (k_cnt2), 3 a recount of the retained level-1 records */
} yakamd_stats_t;
int yakamd_get_stats(yak_ch_t *h, yakamd_stats_t *st);

#ifdef __cplusplus
}
#endif
#endif
