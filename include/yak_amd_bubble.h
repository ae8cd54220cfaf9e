/* yak_amd_bubble.h -- the simple bubbles of the compacted de Bruijn graph of a count table called on the GPU (libyak_amd_bubble.so; not in the
 * reference).
 *
 * A layer above libyak_amd_gfa.so, libyak_amd_walk.so and libyak_amd.so: it consumes the descriptors and the bases of a device walk
 * (include/yak_amd_walk.h) and the links of include/yak_amd_gfa.h (section 22), and nothing else.  All definitions -- unitig,
 * its order j, its bases S_j, open unitig and cycle, oriented end, link and the order of the list -- are those of the three headers below.
 *
 * An oriented end is e = j << 1 | o (o = 1 for '-'), as in yakamd_ulink_t.  out(e) is the links with from == e in list order (by the base A, C, G,
 * T they append), deg(e) = |out(e)|; the list holds the mirror of every link, so deg(e ^ 1) links arrive at e.
 * A simple bubble is (s, a1, a2, t): s is an oriented end of an open unitig with deg(s) == 2 and out(s) = [a1, a2]; a1 >> 1 != a2 >> 1 and neither
 * is the unitig of s; for both arms deg(a ^ 1) == 1 and deg(a) == 1; out(a1)[0] == out(a2)[0] == t; deg(t ^ 1) == 2; t >> 1 is neither arm's
 * unitig (t >> 1 == s >> 1 is allowed: a circular sequence with one SNP).  Every bubble is seen from s and from t ^ 1 and is reported once, from
 * the side with s < (t ^ 1); the bubbles are listed by s ascending.
 * With A_i the oriented string of arm i (S_j, or its reverse complement for '-') and n_i its n_node: type S (YAKAMD_BUBBLE_S) if n_1 == n_2 == k
 * -- the arms then differ in the one base at index k - 1 --, E if n_1 == n_2 != k, I otherwise; hd = the Hamming distance of A_1 and A_2 when
 * n_1 == n_2, else ~0.  The allele of an arm is A_i[k - 1 : n_i], n_i - k + 1 bases, `*` when that is not positive.
 * A tip is an open unitig with n_node < k one of whose two oriented ends has no link and the other at least one; tips are tallied (n_tip, and
 * tip_nodes = the sum of their n_node), not listed.  n_fork = the oriented ends of open unitigs with deg >= 2; max_arm_nodes = the largest n_node
 * of an arm of a bubble.
 *
 * yakamd_bubble_open(): copies of the walk's descriptors and bases and of the links are taken through the getters (neither the walk nor the links
 * are needed afterwards), the run of links of every end is found, every oriented end decides whether it reports a bubble, the bubbles are written
 * at their rank and classified; the records stay in device memory until yakamd_bubble_close().  The work is done on the device that is current at
 * the call, which stays current.  NULL after a message (yakamd_bubble_last_error()), before any device work: w or g is NULL; k is even or outside
 * [3, 31]; k does not fit the walk (sum_len != n_node + (n_open + n_cycle) (k - 1)); the walk and the links disagree in the number of unitigs.
 * NULL as well, after the first kernel, for a list of links that is not sorted by `from`, names an end outside the unitigs or gives an end more
 * than 4 links.  A walk without unitigs opens and has no bubble.
 * yakamd_bubble_records_dev() copies into device memory of the caller (cap in entries, 16-byte aligned) and returns the number of bubbles; with a
 * NULL pointer or a smaller cap the number needed, and nothing is written.  -1 after a message. */
#ifndef YAK_AMD_BUBBLE_H
#define YAK_AMD_BUBBLE_H
#include "yak_amd_gfa.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { YAKAMD_BUBBLE_S = 0, YAKAMD_BUBBLE_E = 1, YAKAMD_BUBBLE_I = 2 };

typedef struct yakamd_bubble_set yakamd_bubble_set_t;
typedef struct { uint64_t src, sink, arm[2], n_node[2], kc[2], hd, type; } yakamd_bubble_t;      /* 80 bytes */
typedef struct { uint64_t n_bubble, n_type[3], n_tip, tip_nodes, max_arm_nodes, n_fork; } yakamd_bubstat_t;

yakamd_bubble_set_t *yakamd_bubble_open(yakamd_uwalk_t *w, yakamd_gfa_t *g, int k);   /* borrows both; records stay in device memory until close */
int     yakamd_bubble_stats(yakamd_bubble_set_t *b, yakamd_bubstat_t *st);
int64_t yakamd_bubble_records_dev(yakamd_bubble_set_t *b, void *d, int64_t cap);      /* n_bubble entries */
void    yakamd_bubble_close(yakamd_bubble_set_t *b);

/* `yak-amd bubbles` as a library call: the device walk at o->min_cnt, the links, the bubbles, and the text made on the host -- a first line
 * `#bubbles k=<k> min_cnt=<c>`, then per bubble in list order
 * `B <i> u<s><+|-> u<a1><+|-> u<a2><+|-> u<t><+|-> <S|E|I> <n1> <n2> <hd or .> <kc1> <kc2> <allele1> <allele2>`, the u<j> being the names of the
 * S lines of yakamd_unitigs_gfa(); with stats_only the text of yakamd_unitigs_gfa() with stats_only followed by the line
 * `B n_bubble n_S n_E n_I n_fork n_tip tip_nodes max_arm_nodes`.  All fields are separated by tabs; n_threads and batch_keys of the options are
 * ignored.  0, or -1 after a message on stderr -- on a refusal before the output is created */
int     yakamd_bubbles(const yakamd_ugopt_t *o, yak_ch_t *ch, const char *out_fn);
/* measurement: the milliseconds the calling thread's last yakamd_bubble_open / yakamd_bubbles call spent on the copies of the walk's results and the
 * links, the first link of every end, the find (count, scan and emit), the classification, the text (with the copies out) */
void    yakamd_bubble_ms(double ms[5]);
const char *yakamd_bubble_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_gfa_tally_names / _read / _reset are for libyak_amd_gfa.so's */
int  yakamd_bubble_tally_names(const char *const **names);
void yakamd_bubble_tally_read(uint64_t *out, int n);
void yakamd_bubble_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
