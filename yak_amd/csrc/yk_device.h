/*
 * yk_device.h -- shared declarations between the HIP kernels (kernels.hip) and the host engine
 * (engine_*.cpp).  Internal; the public surface is include/yak.h + include/yak_amd.h.
 */
#ifndef YK_DEVICE_H
#define YK_DEVICE_H

#include <stdint.h>
#include <hip/hip_runtime.h>
#include "replay_plan.h"                 /* u32 / u64, YK_NOCAP, and the parameter blocks of the layout replay: ReplayTask, R2Tab, R2Act, R2Load, R2Pub */

typedef ulonglong2 Rec;                  /* one k-mer instance: .x = yak_hash64 value, .y = stream position (32 bits used) */

#define YK_EMPTY   0xFFFFFFFFFFFFFFFFull     /* unclaimed slot (accumulator and table image) */
#define YK_TINF    0xFFFFFFFFFFFFFFFFull     /* "never" */
#define YK_FLAG_FP 1u                        /* first occurrence passed the bloom gate */

/* Tagged 8-byte level-1 record (k < 32, 2k - pre <= 52): (hash >> pre) << 12 | toggle << 10 | position inside the 1024-position
 * round of the partitioning workgroup.  Inside a bucket the records of one round are contiguous and the rounds follow each other in
 * stream order (the write combining is stable at round granularity); the toggle bit flips between consecutive rounds that
 * contributed to the bucket, across workgroups too (the histogram sweep counts them), so the level-2 partition recovers every
 * record's rank in the sub-table's stream: the "time" that orders put-calls.  Stream positions are not stored at all. */
#define YK_R8_TAG_BITS 12
#define YK_R8_TOGGLE   (1u << 10)

#include "rec_fmt.h"                     /* RecFmt: what a buffer of level-1 records holds -- Rec, the tagged record above, the hash, the range-tagged hash */
static inline size_t yk_rec_bytes(RecFmt f) { return f == YK_FMT_POS ? sizeof(Rec) : 8; }
static inline size_t yk_rec_units(RecFmt f, size_t n) { return (n * yk_rec_bytes(f) + sizeof(Rec) - 1) / sizeof(Rec); }   /* elements of a DevBuf<Rec> that hold n records */
extern "C" int64_t yk_knob(const char *name, int64_t dflt);   /* pool.cpp: a run-time setting -- the test hook's value (yakamd_test_set), else (public names only) the environment's, else dflt */
/* tagged records fit this k and prefix: a one-word hash whose bits above `pre` leave the tag its room, and no more buckets than k_xpart_wcs takes */
static inline bool yk_tagged_fits(int k, int pre) { return k < 32 && 2 * k - pre <= 64 - YK_R8_TAG_BITS && pre <= 10 && yk_knob("YAKAMD_REC8", 1) != 0; }

/* the inverse of yak_hash64 (reference yak-priv.h:41-68): one definition for the host (yak_ch_getseq) and the device (kern_print.inc) */
__host__ __device__ static inline u64 yk_hash64_inv(u64 x, u64 m)
{
	u64 t;
	t = x - (x << 31); x = (x - (t << 31)) & m;
	t = x ^ x >> 28; x = x ^ t >> 28;
	x = (x * 14933078535860113213ULL) & m;
	t = x ^ x >> 14; t = x ^ t >> 14; t = x ^ t >> 14; x = x ^ t >> 14;
	x = (x * 15244667743933553977ULL) & m;
	t = x ^ x >> 24; x = x ^ t >> 24;
	t = ~x; t = ~(x - (t << 21)); t = ~(x - (t << 21)); x = ~(x - (t << 21)) & m;
	return x;
}

/* accumulator slot: one per distinct hashed k-mer seen by the current pass (32 B, one sector) */
struct __attribute__((aligned(32))) AccSlot {
	u64 key;        /* full yak_hash64 value, YK_EMPTY if free */
	u64 t1;         /* stream position of the first occurrence  (atomicMin) */
	u64 t2;         /* stream position of the second occurrence (atomicMin of the losers) */
	u32 cnt;        /* occurrences (exact up to 2^32-1, clamped to 1023 on output) */
	u32 flags;
};

struct AccTab {
	AccSlot *s;
	u64 mask;       /* capacity - 1 */
	int bits;       /* log2 capacity, >= pre + 1 */
	int pre;
};

/* device-resident image of the 1<<pre khashl tables (exact layout) */
struct ImgView {
	const u32 *bits;    /* [P] log2 capacity or YK_NOCAP */
	const u64 *off;     /* [P] first slot in the arena (multiple of 32) */
	u64 *keys;          /* arena: (hash>>pre)<<10 | count, YK_EMPTY in unused slots */
	u32 *used;          /* arena bitmap, bit i <-> arena slot i */
	u32 *delta;         /* per-slot pending count increments of the running pass (may be 0) */
	int pre;
	int k;
};

/* bloom geometry (reference bbf.c): per sub-table 1<<nb bits in 512-bit blocks */
struct BloomView {
	u32 *bits32;        /* P << (nb-5) words */
	int nb;             /* log2 bits per sub-table (= bf_shift - pre) */
	int n_hash;
	int mw;             /* u64 words of a "missing probes" mask */
};

#ifdef __cplusplus
extern "C" {
#endif

/* ---- launch wrappers implemented in kernels.hip (all asynchronous on `st`) ---- */
void yk_launch_extract(const uint8_t *bases, int64_t pos0, int64_t n, int64_t t_sub, int k, int pre, int plo, int phi,
                       u64 *out_hash, u32 *out_t, u64 *cursor, hipStream_t st);
void yk_launch_pack(const uint8_t *a, int64_t n, u32 *codes, u32 *valid, hipStream_t st);
/* the level-1 partition of the k-mers ending at [pos0, n): records of any RecFmt to `out`, grouped by their nb_bits-bit prefix; bucket starts and record count to
 * bstart[0 .. 1 << nb_bits].  YK_FMT_TAGGED and YK_FMT_HASH_RNG need k < 32, nb_bits <= 10 (the caller checks).  valid != 0: `bases` is the packed 2-bit image */
void yk_launch_xpart(const uint8_t *bases, int64_t pos0, int64_t n, int64_t t_sub, int k, int pre, int plo, int phi,
                     int nb_bits, u32 *rows, u64 *partial, u64 *bstart, void *out, RecFmt fmt, hipStream_t st, const u32 *valid = 0);
void yk_launch_rpart(const u64 *in_hash, const u32 *in_t, int64_t n, int pre, int plo, int phi,
                     int nb_bits, u32 *rows, u64 *partial, u64 *bstart, Rec *out, hipStream_t st);
int yk_xpart_blocks(int64_t n_pos);
int yk_part_groups(void);
int yk_rpart_blocks(int64_t n_rec);
int yk_bad_hash_seen(hipStream_t st);
void yk_par_counters(u32 *ok, u32 *fail);
void yk_replay_prof(u64 *out8);
void yk_launch_acc_init(AccSlot *s, u64 n, hipStream_t st);
void yk_launch_acc_insert(const Rec *rec, int64_t n, u64 t0, AccTab tab, ImgView img,
                          int img_nonempty, int bloom_mode, u64 *newlist, u64 *counters, hipStream_t st);
void yk_launch_acc_rehash(AccTab oldt, AccTab newt, hipStream_t st);
void yk_launch_img_count(const Rec *rec, int64_t n, ImgView img, hipStream_t st);
size_t yk_img_count_lds_bytes(u32 cap, u32 count);
void yk_launch_lookup(const uint8_t *bases, int64_t n, int k, ImgView img, void *out, int width, hipStream_t st);   /* width 1 (triobin): clears the flag yk_tb_over_seen() reads */
void yk_launch_qv_reduce(const unsigned short *t, const u64 *roff, const u32 *rlen, int64_t n_reads, int min_len, double min_frac,
                         u32 *tot_out, u32 *non0_out, u64 *hist, hipStream_t st);
int yk_tb_over_seen(hipStream_t st);
/* yak inspect's join (kern_inspect.inc): J[c0 * 1024 + c1] += 1 per key of A's sub-tables [sub_lo, sub_lo + n_sub) (keys / off / hdr as
 * InArgs), probed in B's image on its sub-tables [blo, bhi) (has_b = 0: c1 = 0); 0, or -1 if the launch failed */
int yk_launch_inspect(const u64 *keys, const u64 *off, u64 n, int n_sub, int sub_lo, int hdr, int pre_a, int has_b, ImgView img, int blo, int bhi,
                      int ref, u64 *J, hipStream_t st);
/* yak print's listing (kern_print.inc) of the n keys of sub-tables [sub_lo, sub_lo + n_sub) in `img`, the .yak body yk_ctx_dump_image_dev() makes
 * of them; off[j] = keys before sub-table sub_lo + j (n_sub + 1 words, off[n_sub] = n).  kmers: x[i] and c[i] of key i.  print: the lines of reference
 * main.c:308-317 to `text`; with counts, tile_bytes[t] = bytes of tile t's lines (print_sizes) and tile_off their exclusive scan (yk_print_tiles(n) + 1
 * words).  0, or -1 if the launch failed */
u64 yk_print_tiles(u64 n);
int yk_launch_kmers(const u64 *img, const u64 *off, u64 n, int n_sub, int sub_lo, int k, int pre, u64 *x, unsigned short *c, hipStream_t st);
int yk_launch_print_sizes(const u64 *img, const u64 *off, u64 n, int n_sub, int k, u32 *tile_bytes, hipStream_t st);
int yk_launch_print(const u64 *img, const u64 *off, u64 n, int n_sub, int sub_lo, int k, int pre, int with_counts, const u64 *tile_off,
                    uint8_t *text, hipStream_t st);
void yk_launch_tb_reduce(const uint8_t *flag, const u64 *roff, const u32 *rlen, int64_t n_reads, int k, int *cnt, hipStream_t st);
int64_t yk_te_tiles(int64_t n);                               /* trioeval's streak reduction (kern_trioeval.inc) */
int64_t yk_te_keep_blocks(int64_t n_runs);
/* low = 0: trioeval's flags (2 -> type 1, 8 -> type 2); low = 1: chkerr's low bytes (1 -> type 1) */
void yk_launch_te_runs(const uint8_t *flag, int64_t n, u32 *tcnt, const u64 *toff, u64 *st, u64 *en, int scatter, hipStream_t s, int low = 0);
void yk_launch_te_scan(const u32 *cnt, int64_t m, int n_arrays, u64 *off, hipStream_t s);
void yk_launch_te_keep(const u64 *st, const u64 *en, const uint8_t *flag, int64_t n_runs, int min_n, u32 *kcnt, const u64 *koff,
                       const u64 *seq_off, int64_t n_seq, void *list, int scatter, hipStream_t s, int low = 0);
void yk_launch_te_seq(const void *list, const u64 *n_list, int64_t n_max, int k, int *cnt6, hipStream_t s);
/* yak chkerr's lookup (kern_extract.inc): out[i] = 1 where yak_ch_get() < min_cnt (-1 when absent), 0 where not, 0xff where no k-mer ends */
void yk_launch_ce_lookup(const uint8_t *bases, int64_t n, int k, ImgView img, uint8_t *out, int min_cnt, hipStream_t st);
/* yak sexchr's tally (kern_trioeval.inc): cnt[4 j ..] += n_k, n_sexchr, n_sex1, n_sex2 of record j over the flags (zeroed by the caller) */
void yk_launch_sc_reduce(const uint8_t *flag, int64_t n, const u64 *seq_off, const u32 *seq_len, int64_t n_seq, u64 *cnt, hipStream_t s);
/* `yak-amd depth` (kern_depth.inc): the windows of a u16 count array.  DpArgs: the array of n_bytes elements, sequence j at seq_off[j] with seq_len[j]
 * positions, win_off[j] = windows of the sequences before j (n_seq + 1 words), w = k-mer starts per window (0: one window per sequence) */
struct DpArgs { const unsigned short *cnt; const u64 *seq_off; const u32 *seq_len; const u64 *win_off; int64_t n_seq, n_bytes; u64 w; int k; };
int yk_dp_run(void);                                          /* positions of a long window per tile */
void yk_launch_dp_short(DpArgs a, u64 g0, u32 n_win, u32 T, void *out, u32 *long_list, u64 *tile_base, u32 long_cap, u64 *counter, hipStream_t st);
void yk_launch_dp_long(DpArgs a, u64 g0, const u32 *long_list, const u64 *tile_base, u32 slot0, u32 n_slots, u64 tile0, u64 n_tiles, u64 *hist, hipStream_t st);
void yk_launch_dp_finish(const u64 *hist, const u32 *long_list, u32 slot0, u32 n_slots, void *out, hipStream_t st);
/* `yak-amd cover` (kern_cover.inc): one pass over the u16 count array t of n positions.  cov[i] = 1 where base i lies inside a k-mer whose count
 * min(t, 1023) is in [lo, hi], else 0; with mask 1 / 2 `masked` = `bases` with the covered letters in lower case / the covered bytes as 'N'; tally[4 j ..]
 * += n_kmer, n_hit, n_cov, n_run of sequence j (zeroed by the caller; n_seq = 0: no tally).  cov and masked are written up to the next multiple of 16 */
struct CvArgs {
	const unsigned short *t; int64_t n;
	const u64 *seq_off; const u32 *seq_len; int64_t n_seq;
	const uint8_t *bases; uint8_t *cov, *masked; u32 *tally;
	int k; u32 lo, hi;
};
int64_t yk_cover_tile(void);                                  /* positions per tile, and per workgroup */
int64_t yk_cover_group(void);
void yk_launch_cover(CvArgs a, int mask, hipStream_t st);
/* `yak-amd hetmers` (kern_hetmer.inc): the middle-base neighbours of the n keys of sub-tables [sub_lo, sub_lo + n_sub) (keys / off as yk_launch_kmers
 * takes them), probed in the whole image `img` (k odd, below 32); a key below min_cnt is absent.  mode 0: group[s] += groups of s members, J[lo * 1024
 * + hi] += 1 per pair; mode 1: tile_cnt[t] = pairs of tile t (yk_hetmer_tiles(n) words); mode 2: the 24-byte records {x, y, cx, cy} of tile t from
 * list[tile_off[t]] on (tile_off = the exclusive scan of tile_cnt).  0, or -1 if the launch failed */
u64 yk_hetmer_tiles(u64 n);
int yk_launch_hetmer(int mode, const u64 *keys, const u64 *off, u64 n, int n_sub, int sub_lo, int min_cnt, ImgView img, u64 *J, u64 *group,
                     u32 *tile_cnt, const u64 *tile_off, void *list, hipStream_t st);
/* `yak-amd unitigs` (kern_graph.inc): the de Bruijn graph of the whole image `img` (k odd, below 32; a key below min_cnt is absent).  A tile is
 * yk_graph_tile() consecutive slots of one sub-table; tile0[p] / key0[p] = the tiles / stored keys of the sub-tables before p (P + 1 words each).
 * what 0: edges[slot] = the edge mask of the slot's key and tally[l * 5 + r] += nodes of l left and r right edges, `inflight` (4, or 8) probes at a
 * time; 1: wrank[w] = used slots of the sub-table in front of word w; 2: tally[25] += linked sides; 3: the 32-byte records of the keys of tiles
 * [t_lo, t_hi) to out[listing index - out_key0], out_n of them.  grid_want > 0: that many workgroups.  0, or -1 if the launch failed */
u64 yk_graph_tile(void);
int yk_launch_graph(int what, int inflight, int grid_want, const u64 *tile0, const u64 *key0, uint8_t *edges, u32 *wrank, u64 *tally, u64 t_lo, u64 t_hi, u64 n_slots,
                    int P, int min_cnt, void *out, u64 out_key0, u64 out_n, ImgView img, hipStream_t st);
/* homopolymer compression of a base image (kern_hpc.inc).  valid == 0: `in` is the ASCII image, valid != 0: the packed one.  Three
 * launches: the kept positions per tile of yk_hpc_tile(packed) positions into tcnt (yk_hpc_tiles() words), their exclusive scan into toff
 * (yk_launch_te_scan, one word more: toff[tiles] = the output's length), the kept bytes to `out` with '\n' up to the next multiple of 16.
 * yk_launch_hpc_remap(): off_out / len_out of n_seq sequences of the ASCII image from its toff */
int64_t yk_hpc_tile(int packed);
int64_t yk_hpc_tiles(int packed, int64_t n);
void yk_launch_hpc_count(const void *in, const u32 *valid, int64_t n, u32 *tcnt, hipStream_t st);
void yk_launch_hpc_scatter(const void *in, const u32 *valid, int64_t n, const u64 *toff, uint8_t *out, hipStream_t st);
void yk_launch_hpc_remap(const uint8_t *a, int64_t n, const u64 *toff, const u64 *off, const u32 *len, int64_t n_seq, u64 *off_out, u32 *len_out, hipStream_t st);
int yk_launch_img_count_lds(const void *rec, RecFmt fmt, const u64 *bstart, ImgView img, int plo, int phi, size_t lds, u64 *compact, u32 stride, hipStream_t st);
void yk_launch_img_count_h(const u64 *hash, int64_t n, ImgView img, hipStream_t st);
void yk_launch_img_inc(ImgView img, u64 hash, u64 *out2, hipStream_t st);
void yk_launch_img_fold(ImgView img, u64 n_slots, hipStream_t st);
void yk_launch_img_hist(ImgView img, u64 n_slots, u64 *hist, hipStream_t st);
void yk_launch_img_setcnt(ImgView img, u64 n_slots, u32 cnt, hipStream_t st);
void yk_launch_img_clear(ImgView img, u64 n_slots, hipStream_t st, int bump = 0);   /* bump: every count + 1, saturating, instead of 0 */
void yk_launch_lastput(const Rec *rec, int64_t n, u64 t0, u64 t_from, AccTab tab, ImgView img,
                       int img_nonempty, int bloom_mode, const u32 *only_missing, u64 *lp_batch, hipStream_t st);
void yk_launch_lastput_merge(u64 *lastput, const u64 *lp_batch, u32 *missing, u32 *n_missing, int P, int plo, int phi, hipStream_t st);

void yk_launch_bf_test(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, u64 *miss, hipStream_t st);
void yk_launch_bf_set(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                      u32 *multi, int multi_bits, u64 *counters, hipStream_t st);
void yk_launch_bf_check(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                        const u32 *multi, int multi_bits, u64 *cand, u64 *counters, hipStream_t st);
void yk_launch_bf_mapfill(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                          const u32 *multi, int multi_bits, u64 *map, int map_bits, hipStream_t st);
void yk_launch_bf_resolve(AccTab tab, const u64 *newlist, const u64 *cand, u64 n_cand, BloomView bf,
                          const u64 *miss, const u64 *map, int map_bits, hipStream_t st);

void yk_launch_select_count(AccTab tab, int bloom_mode, int P, u32 *seg_cnt, hipStream_t st);
void yk_launch_select_scatter(AccTab tab, int bloom_mode, int P, const u64 *seg_off, u32 *seg_cur,
                              u64 *rec_kc, u64 *rec_t, hipStream_t st);
void yk_launch_seg_sort_pass(const u64 *seg_off, int P, const u64 *src_kc, const u64 *src_t,
                             u64 *dst_kc, u64 *dst_t, int shift, u32 *dig_hist, int n_dig, hipStream_t st);
void yk_launch_replay(const ReplayTask *tasks, int n_tasks, int n_threads, const u64 *old_keys, const u32 *old_used,
                      u64 *new_keys, u32 *new_used, u32 *scr_used, u32 *scr_owner, u64 *scr_par,
                      const u64 *rec_kc, const u64 *rec_t, const u64 *lastput,
                      u32 *out_bits, u32 *out_count, u32 lds_words, hipStream_t st);
int yk_shrink_shares(void);
void yk_launch_shrink_count(ImgView img, int P, int cmin, int cmax, int which, ImgView other, u32 *seg_cnt, hipStream_t st, int rng = 0);
void yk_launch_shrink_scatter(ImgView img, int P, int cmin, int cmax, int which, ImgView other, const u64 *seg_off, u64 *rec_kc, hipStream_t st, const u32 *rng_cnt = 0);
struct ResizeTask { u32 old_bits, new_bits, rehash, pad; u64 old_off, new_off; };
void yk_launch_resize(const ResizeTask *tasks, int P, const u64 *old_keys, const u32 *old_used, u64 *new_keys, u32 *new_used, u32 *scr_used, hipStream_t st);
void yk_launch_keys_to_hashes(const u64 *kc, const u64 *seg_off, int P, int pre, u64 *hash, u32 *t, hipStream_t st, unsigned short *cnt = 0);   /* cnt != 0: the keys' counts as well */
void yk_launch_img_add_counts(const u64 *hash, const unsigned short *cnt, u64 n, ImgView img, int plo, int phi, u32 *missing, hipStream_t st);
void yk_launch_put_u64(const u64 *pos, const u64 *val, u32 n, u64 *out, hipStream_t st);

#ifdef __cplusplus
}
#endif

/* counters[] layout (u64 each) */
enum { YKC_NEW = 0, YKC_INST = 1, YKC_ANYMULTI = 2, YKC_NCAND = 3, YKC_NMARKED = 4, YKC_EXIST = 5, YKC_N = 8 };


/* ---------------- fast path (exclusive-ownership LDS counting) ---------------- */
#define YK_CH2     32768            /* records per level-2 partition chunk */
#define YK_LDS_C   1024             /* slots of the LDS counting table (overflow beyond 768 distinct k-mers) */

struct Chunk2 {                     /* one level-2 partition work item: a run of one level-1 bucket */
	const Rec *rec;
	u64 spare;
	u32 n, bucket;
	u32 tbase;                      /* added to tlo: time relative to the start of the pass */
	u32 fmt;                        /* RecFmt of the chunk: YK_FMT_POS, or YK_FMT_TAGGED (tbase = records of this bucket in earlier batches) */
	u32 before, after;              /* YK_FMT_TAGGED: records of the same bucket of the same batch lying before / behind the chunk in memory */
};

struct FastParams {
	int pre, k, s2_bits;            /* sub-buckets per sub-table = 1 << s2_bits */
	int bloom_mode, nb, n_hash;     /* nb = log2 bits per sub-table filter */
	int img_nonempty;
	int plo, phi;
	int dbg, bf_virgin;             /* dbg: timing ablations only (YAKAMD_DBG); bf_virgin: filter never written (all zero) */
	int rec8_in, rec8_out, tb;      /* level-2 input is tagged 8-byte records; its output (the counting kernels' input) is 8 bytes: (hash >> pre minus the sub-bucket bits) << tb | rank, tb = 12 + s2_bits */
	int or_mode;                    /* loads from a .yak file (htab.c:436-470) instead of counting: 1 = the low 4 bits of a record's time are a flag, ORed into the key's low bits; 2 = the low 10 bits are the saved count, kept by new keys only */
	/* which bits of x = hash >> pre name the sub-bucket: the top s2_tot bits of x's low `sw` bits (sw = log2 bloom blocks per sub-table with a filter -- a
	 * sub-bucket owns a contiguous range of blocks -- else sw = s2_tot).  A partition sweep routes by s2_bits of them: ((x mod 2^sw) >> ssh) mod 2^s2_bits.
	 * One sweep does them all (ssh = sw - s2_tot, s2_bits = s2_tot: the counting kernels always see this form); beyond 2^13 sub-buckets per sub-table a
	 * first sweep takes the high s2_tot - 11 bits (ssh = sw - s2_bits) and a second one, on the groups of the first, the low 11 (ssh = sw - s2_tot) */
	int sw, ssh, s2_tot;
	int bf_nowb;                    /* k_lc2: the staged filter ranges are not written back (the caller keeps every record of the pass and rebuilds the filter from them if anything ever reads it: k_bf_rebuild) */
	u64 t_pass0;
};

/* outputs of the exclusive-ownership counting kernels: the keys a sub-bucket adds to its sub-table go to the
 * front of the sub-bucket's own record range in kc / T (fragments, gathered by k_lc_compact); per sub-bucket
 * their number, the time (relative to the slice, + 1; 0 = none) of its last put-call, its distinct k-mers.
 * c2 (0 = not wanted): next to every selected key, min(instances of the key in the sub-bucket's records, 1023) -- what a count pass over the
 * same records adds to it (engine_slice.cpp keep2: that pass then only applies these, k_cnt2_apply) */
struct LcOut { u64 *kc, *T; u32 *nsel, *lp, *nd; unsigned short *c2; };

#ifdef __cplusplus
extern "C" {
#endif
int yk_rng_log(void);
int yk_hpart2_chunk(void);
void yk_launch_hpart2(const Chunk2 *chunks, int n_chunks, const u32 *chunk_first, const u64 *bbase, ImgView img, int rb, int P,
                      u32 *rows2, u64 *sbstart, u64 *out, hipStream_t st);
int yk_launch_img_count_rng(const u64 *rec, int cross, const u64 *sbstart, ImgView img, int plo, int phi, int rb, u32 max_len,
                            u64 *list, u32 *list_n, u32 list_cap, hipStream_t st);
void yk_launch_part2(const Chunk2 *chunks, int n_chunks, const u32 *chunk_first /*[P+1]*/, const u64 *bbase, FastParams fp, int P,
                     u32 *rows2, u64 *sbstart, Rec *out, hipStream_t st);
void yk_launch_lds_count_ovf(FastParams fp, const u64 *sbstart, const Rec *rec,
                             u32 *bloom32, ImgView img, LcOut O, const u32 *ovf_list, u32 n_ovf, const u64 *scr_off,
                             u64 *scr, hipStream_t st);
/* replay2 (layout replay of large sub-tables, kernels.hip; its parameter blocks: replay_plan.h) */
void yk_r2_binit(const R2Tab *tabs, const R2Act *acts, int P, u32 bmax, u32 *OCC, u32 *USED, hipStream_t st);
void yk_r2_dsmall(const R2Tab *tabs, const R2Act *acts, int P, u64 *K0, u64 *K1, u32 *TAG, u32 *OCC, u32 *USED, u32 *Fcur, u32 *Gcur, u32 *fail, hipStream_t st);
int yk_r2_double(const R2Tab *tabs, const R2Act *acts, int P, int n_dbl, u64 *K0, u64 *K1, u32 *TAG, u32 *OCC, u32 *USED, const u32 *Fin, u32 *Fout, u32 *fail, hipStream_t st);
void yk_r2_place(const R2Tab *tabs, const R2Act *acts, int P, int p0, int np, u32 bmax, u64 *K0, u64 *K1, const u64 *kc, u64 *pk, u32 *pr, u32 *seg_start,
                 u32 *head, u64 *spill, u32 *spill_n, u32 spill_cap, u32 *fail, u32 *img_u, const u32 *USED, u32 *pcnt, int G, hipStream_t st);
void yk_r2_load(const R2Tab *tabs, const R2Load *ld, int P, u32 bmax, const u64 *src1, const u64 *src2, u64 *K0, u64 *K1, u32 *USED, hipStream_t st);
void yk_r2_trail(const u64 *lastput, const u64 *rec_t, const u64 *rec_off, const u32 *m, int P, u32 *out, hipStream_t st);
void yk_r2_publish(const R2Tab *tabs, const R2Pub *pub, int P, u32 bmax, const u64 *K0, const u64 *K1, u64 *nk, u32 *nu, hipStream_t st);
int yk_r2_small_f(void);
int yk_r2_seg_log(void);
int yk_r2_head(void);
size_t yk_count_own_lds(u32 range_len, u32 kmax);
int yk_launch_img_count_own(const void *rec, RecFmt fmt, int cross, const u64 *bstart, ImgView img, int plo, int phi, int rb, int rng_log, u32 kmax,
                            size_t lds, u64 *list, u32 *list_n, u32 list_cap, hipStream_t st);
int yk_lc2_ok(FastParams fp);
int yk_lc2_per_sb(int bloom_mode);
void yk_launch_lc2(FastParams fp, const u64 *sbstart, const Rec *rec, u32 *bloom32, ImgView img, LcOut O, u64 *counters, u32 *ovf_list, hipStream_t st);
void yk_launch_lc_sum(const u32 *nsel, int s2_bits, int plo, int phi, u32 *seg_cnt, hipStream_t st);
void yk_launch_lc_compact(LcOut O, const u64 *sbstart, int s2_bits, int plo, int phi, u64 t_pass0, const u64 *seg_base,
                          u64 *out_kc, u64 *out_T, u64 *lastput, u32 *ndist_p, Rec *out_kt, u32 *out_c2, hipStream_t st);
void yk_launch_part2_ts(const Chunk2 *chunks, int n_chunks, const u32 *chunk_first, const u64 *bbase, FastParams fp, int P, u32 *rows2, u64 *sbstart, Rec *out, hipStream_t st);
int yk_launch_ts_rank(const u64 *binstart, const Rec *in, int w, int j, u32 bin_lo, u32 n_bins, u64 *out_kc, u64 *out_t, u32 *fail, hipStream_t st);
void yk_launch_kt_split(const Rec *in, u64 n, u64 *out_kc, u64 *out_t, hipStream_t st);
void yk_launch_bf_rebuild(FastParams fp, const u64 *sbstart, const Rec *rec, u32 *bloom32, hipStream_t st);
void yk_launch_lc_sum3(LcOut O, int s2_bits, int plo, int phi, u64 t_pass0, u32 *seg_cnt, u64 *lastput, u32 *ndist_p, hipStream_t st);
void yk_launch_lc_gather(LcOut O, const u64 *sbstart, const u64 *key_off, int s2_bits, int plo, int phi, u64 *out_kc, u64 *out_T, Rec *out_kt, u32 *out_c2, hipStream_t st);
void yk_launch_cnt2(FastParams fp, const u64 *sbstart, const Rec *rec, const u64 *key_off, const u64 *key_kc, const u64 *seg_base, u32 *key_cnt, ImgView img, u64 n_keys, u32 *used_delta, hipStream_t st);
void yk_launch_cnt2_apply(FastParams fp, const u64 *key_kc, const u32 *key_cnt, const u64 *seg_base, ImgView img, hipStream_t st, int fix = 0);   /* fix: behind k_img_clear's bump */
void yk_launch_nsel_scan(const u32 *nsel, int s2_bits, int plo, int phi, int P, const u64 *seg_base, u64 *key_off, hipStream_t st);
void yk_launch_seg_sort_pass2(const u64 *seg_base, const u32 *seg_cnt, int P, const u64 *src_kc, const u64 *src_t,
                              u64 *dst_kc, u64 *dst_t, int shift, u32 *dig_hist, int n_dig, hipStream_t st, int big);
#ifdef __cplusplus
}
#endif
enum { YKC_NOVF2 = 7 };               /* sub-buckets k_lc2 passed on to the tier behind it */

#endif
