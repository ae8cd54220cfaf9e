/* yak_amd_clean.h -- the compacted de Bruijn graph of a count table cleaned on the GPU: tips clipped, simple bubbles popped, round by round
 * (libyak_amd_clean.so; not in the reference).
 *
 * A layer above libyak_amd_bubble.so, libyak_amd_gfa.so, libyak_amd_walk.so and libyak_amd.so: it consumes the descriptors and the bases of a device
 * walk (include/yak_amd_walk.h), the links of include/yak_amd_gfa.h and the records of include/yak_amd_bubble.h, decides which unitigs go, and
 * removes their k-mers from the table with public calls of libyak_amd.so alone: the bases of the removed unitigs are written as a base image, one
 * record per unitig, that image is counted into a drop table D (yak_ch_init, yakamd_pass_begin, yakamd_feed_bases_dev, yakamd_pass_end), and
 * yak_ch_subtract(h, D) takes D's k-mers out of h.  The cleaned graph is the graph of the cleaned table: every command that reads a table works
 * on the result.
 *
 * Notation of yak_amd_bubble.h: an oriented end is e = j << 1 | o, out(e) the links with from == e in list order, deg(e) = |out(e)|; n_j and kc_j
 * are n_node and kc of unitig j.
 * Coverage order: j is stronger than j' iff kc_j n_j' > kc_j' n_j, or the two products are equal and j < j'.  The products are compared exactly, in
 * 128 bits; there is no floating point.
 * Tip candidate: tipcand(e) for an oriented end of an open unitig iff n_{e >> 1} < tip_nodes, deg(e) == 1 and deg(e ^ 1) == 0.
 * Clipping: unitig j is clipped iff one of its ends e has tipcand(e); with a = out(e)[0], a >> 1 != j; and there is an x in out(a ^ 1), x != e ^ 1,
 * with !tipcand(x ^ 1) or x >> 1 stronger than j.  The strongest of several sibling tips at one anchor stays, and an anchor never loses its last
 * continuation.
 * Popping: for every bubble record (s, a1, a2, t) the loser is the arm that is not the stronger one -- a2 on equal products, whatever the unitig
 * numbers are: the list order decides --, and it is popped iff 100 kc_lo n_hi <= pop_pct kc_hi n_lo.
 * An arm has one link on both sides, so it is no tip, no anchor, no source and no sink; a tip has a side without a link, so it is no anchor: the
 * removed set of a round is the union of all decisions taken on one snapshot and depends on no order.  Cycles are never removed.
 * tip_nodes in [0, 2^20], 0 switches the tips off; pop_pct in [0, 100], 0 switches the bubbles off.
 *
 * yakamd_clean_open() borrows the walk, the links and the bubbles (none is needed afterwards) and keeps, until yakamd_clean_close(), a record per
 * removed unitig ascending by j -- why = YAKAMD_CLEAN_TIP or _POP, other = the anchor end a of a tip or the winning arm's end of a popped arm, off =
 * the exclusive scan of n_node + k -- and the drop image: the removed unitigs' strings in record order, each followed by '\n' (img_bytes bytes).
 * NULL after a message (yakamd_clean_last_error()), before any device work: w, g or b is NULL; k is even or outside [3, 31]; k does not fit the
 * walk; the layers disagree in n_unitig or n_bubble; an option is out of range.  NULL as well, after the kernel that met it, for a list of links, a
 * bubble record or a descriptor that does not fit.  A walk without unitigs opens and removes nothing.
 * The two _dev getters copy into device memory of the caller (cap in entries / bytes, 16-byte aligned) and return the number of entries; with a
 * NULL pointer or a smaller cap the number needed, and nothing is written.  -1 after a message. */
#ifndef YAK_AMD_CLEAN_H
#define YAK_AMD_CLEAN_H
#include "yak_amd_bubble.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { YAKAMD_CLEAN_KEEP = 0, YAKAMD_CLEAN_TIP = 1, YAKAMD_CLEAN_POP = 2 };
#define YAKAMD_CLEAN_MAX_TIP_NODES (1 << 20)

typedef struct yakamd_clean_set yakamd_clean_set_t;
typedef struct { uint64_t unitig, why, n_node, kc, other, off; } yakamd_clean_rec_t;      /* 48 bytes */
/* tips clipped and their nodes, candidates that stay; arms popped and their nodes, bubbles that pop_pct keeps; the records, the bytes of the image */
typedef struct { uint64_t n_tip, tip_nodes, n_tip_kept, n_pop, pop_nodes, n_pop_kept, n_rec, img_bytes; } yakamd_cleanstat_t;
/* a round: the stored keys, unitigs, links and bubbles of its graph, what it decided, the k-mers the table lost */
typedef struct { uint64_t n_key, n_unitig, n_link, n_bubble, n_tip, tip_nodes, n_pop, pop_nodes, removed; } yakamd_cleanround_t;
typedef struct {
	int32_t min_cnt;          /* -c, 1: a k-mer below this count is absent (and is dropped from the table before the first round) */
	int32_t tip_nodes;        /* -t, -1: the table's k */
	int32_t pop_pct;          /* -b, 100 */
	int32_t max_rounds;       /* -r, 8, in [1, 64] */
	int32_t list;             /* -l, 0: a T or P line per removed unitig */
} yakamd_cleanopt_t;
void yakamd_cleanopt_init(yakamd_cleanopt_t *o);

yakamd_clean_set_t *yakamd_clean_open(yakamd_uwalk_t *w, yakamd_gfa_t *g, yakamd_bubble_set_t *b, int k, int tip_nodes, int pop_pct);
int     yakamd_clean_stats(yakamd_clean_set_t *c, yakamd_cleanstat_t *st);
int64_t yakamd_clean_records_dev(yakamd_clean_set_t *c, void *d, int64_t cap);        /* n_rec entries */
int64_t yakamd_clean_image_dev(yakamd_clean_set_t *c, void *d, int64_t cap);          /* img_bytes bytes */
void    yakamd_clean_close(yakamd_clean_set_t *c);

/* one round on a resident table: the device walk at o->min_cnt, the links, the bubbles, the decisions, the drop image, D, the subtraction.  Returns
 * the number of k-mers removed and fills *st (which may be NULL); a round that removes nothing leaves the table untouched and builds no D.  -1
 * after a message.  Whatever the walk refuses stays refused, with its message: a sharded table, a table on several devices, an open pass, an even
 * k, k >= 32 */
int64_t yakamd_clean_round(yak_ch_t *h, const yakamd_cleanopt_t *o, yakamd_cleanround_t *st);
/* `yak-amd clean` as a library call: yak_ch_shrink(ch, min_cnt, 1023) when min_cnt is above 1, rounds until one removes nothing or max_rounds are
 * done, yak_ch_dump(ch, out_yak) and the report to report_fn (NULL: none; "-": stdout), tabs between the fields:
 *   `#clean k=<k> min_cnt=<c> tip_nodes=<T> pop_pct=<P>`
 *   `R <r> <n_key> <n_unitig> <n_link> <n_bubble> <tips> <tip_nodes> <pops> <pop_nodes> <removed>` per round, r from 1
 *   with list, behind each R line in record order: `T <r> u<j> <n_node> <kc> u<anchor><+|->`, `P <r> u<j> <n_node> <kc> u<winner><+|->`
 *   `C <rounds> <n_key_in> <n_key_after_shrink> <n_key_out>`
 * ch is changed: it is the cleaned table afterwards.  0, or -1 after a message -- on a refusal before either output is created */
int     yakamd_clean(const yakamd_cleanopt_t *o, yak_ch_t *ch, const char *out_yak, const char *report_fn);
/* measurement: the milliseconds the calling thread's last yakamd_clean_open / _round / yakamd_clean call spent, summed over its rounds, on the walk,
 * the links, the bubbles, the decisions (with the records), the image, the drop table, the subtraction, the text (with the dump) */
void    yakamd_clean_ms(double ms[8]);
const char *yakamd_clean_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_bubble_tally_names / _read / _reset are for libyak_amd_bubble.so's */
int  yakamd_clean_tally_names(const char *const **names);
void yakamd_clean_tally_read(uint64_t *out, int n);
void yakamd_clean_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
