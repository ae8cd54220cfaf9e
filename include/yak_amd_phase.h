/* yak_amd_phase.h -- the alleles of the simple bubbles phased from read support, on the GPU (libyak_amd_phase.so; not in the reference; DESIGN.md
 * section 32).
 *
 * A layer above libyak_amd_allele.so and the libraries below that: it takes the observation records and the support of include/yak_amd_allele.h
 * (section 31) and nothing else.  A bubble, its index i, its alleles 1 and 2 (a = 0, 1), an observation record, full, and the call het are what
 * that header defines.
 *
 * Fragment: the full observations (flags & YAKAMD_AOBS_FULL) of one sequence of a chunk, in record order: the entries of its F line.  Partial
 * observations take no part.
 * Vote: two neighbouring entries of a fragment with bubbles b1 != b2 and alleles a1, a2 vote on the pair (i, j) = (min, max): cis if a1 == a2, trans
 * otherwise.  Neighbours with b1 == b2 (twice round a circle) give no vote; rev plays no part.  A fragment of n entries gives at most n - 1 votes.
 * Votes are sums over everything fed since the open or the last reset, and do not depend on how the reads are cut into chunks.
 * Edge: with min_sup = m and min_link = e (both at least 1), a pair with cis = c and trans = t is an edge iff both bubbles are het by the call of
 * the support at m and w = |c - t| >= e: a tie is never an edge.  Its parity is x = (t > c).
 * Order: edge E comes before edge F iff w_E > w_F, or w_E == w_F and (i, j)_E is lexicographically smaller: strict and total.
 * Forest: the spanning forest Kruskal's algorithm builds when it takes the edges in that order; it is unique because the order is strict.
 * Block: a connected component of the het bubbles under the edges, named by its smallest bubble index; a het bubble without an edge is a block of one.
 * Phase: h(b) is the XOR of the parities along the forest's path from b to its block's name, so the name has h = 0.  Allele 1 of b lies on
 * haplotype h(b) of its block, allele 2 on the other.  A non-forest edge is concordant iff x == h(i) ^ h(j), discordant otherwise.  Per block:
 * n_bubble, n_edge (all its edges), n_disc, w_sum (over all its edges) and w_disc.
 * Everything is integer, and every result is fixed by these definitions alone, not by the algorithm or by thread timing.
 *
 * yakamd_phase_open(n_bubble): the pair table (16 slots at first) and the per-bubble arrays in device memory of the device current at the call,
 * which is used and stays current in every call below; all device pointers are the caller's.  NULL after a message (yakamd_phase_last_error()) for
 * n_bubble < 0 and n_bubble >= 2^31.  0 bubbles open, and nothing is ever voted.
 * yakamd_phase_votes_dev(): d_obs[0 .. n_obs) as yakamd_allele_obs_dev() wrote the records of one chunk (16-byte aligned); writes n_out =
 * { n_full, n_vote }.  A record whose bubble >= n_bubble, or whose seq is smaller than that of the record before it, is counted, and the call
 * returns -1 after a message and adds nothing.  n_obs == 0 launches nothing.  cis and trans of a pair are 32 bits each: a feed of n_obs records
 * can bring at most n_obs - 1 votes, and one that could bring the votes since the open or the last reset to 2^32 is refused on the host, before
 * any launch (YAKAMD_PHASE_VOTE_LIMIT, a test switch read from the environment, lowers that limit to show the refusal).  The table grows by
 * itself: before a feed's votes, if 2 * (n_pair + n_full) exceeds its capacity, its slots move into a larger one.
 * yakamd_phase_pairs_dev() copies every voted pair as yakamd_ppair_t into device memory of the caller (cap in entries, 16-byte aligned) and
 * returns their number; with a NULL pointer or a smaller cap the number needed, and nothing is written; -1 after a message.  The order of the
 * pairs is the table's slot order, which depends on the capacity and on thread timing: it is not defined.  Compare them as a sorted list.
 * yakamd_phase_solve_dev(): d_sup[0 .. n_sup) as yakamd_allele_support_dev() wrote it (16-byte aligned).  -1 after a message for n_sup !=
 * n_bubble and for a minimum below 1.  It can be called again with other minima on the same votes.
 * yakamd_phase_nodes_dev(), _edges_dev(), _blocks_dev(): the results of the last solve, by the protocol of yakamd_phase_pairs_dev(); -1 after a
 * message before a solve, and after a reset or a feed that was taken behind it, one without a vote included (a refused feed leaves them).  n_bubble nodes: block = ~0 for a bubble that is not het, flags bit 0
 * = h.  The edges: flags bit 0 = x, bit 1 forest, bit 2 discordant; their order is not defined.  The blocks of two bubbles or more, ascending by
 * block.
 * yakamd_phase_reset() sets the votes back to zero; the table keeps its capacity. */
#ifndef YAK_AMD_PHASE_H
#define YAK_AMD_PHASE_H
#include "yak_amd_allele.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { YAKAMD_PEDGE_X = 1, YAKAMD_PEDGE_FOREST = 2, YAKAMD_PEDGE_DISC = 4 };

typedef struct yakamd_phase_tab yakamd_phase_t;
typedef struct { uint32_t i, j, cis, trans; } yakamd_ppair_t;            /* 16 bytes */
typedef struct { uint32_t block, flags; } yakamd_pnode_t;                /* 8 bytes */
typedef struct { uint32_t i, j, w, flags; } yakamd_pedge_t;              /* 16 bytes */
typedef struct { uint32_t block, n_bubble, n_edge, n_disc; uint64_t w_sum, w_disc; } yakamd_pblock_t;      /* 32 bytes */
typedef struct {
	uint64_t n_bubble, n_pair, capacity, n_grow;                         /* the pair table: its keys, its slots, how often it grew */
	uint64_t n_het, n_edge, n_forest, n_block, n_single, n_round;        /* of the last solve; n_block counts the blocks of two or more */
} yakamd_phstat_t;
typedef struct {
	int32_t min_cnt;      /* a k-mer with a count below this is absent, 1 .. 1023 [1] */
	int32_t min_sup;      /* an allele is supported by this many full observations, 1 .. 2^31 - 1 [2] */
	int32_t min_link;     /* a pair is an edge from |cis - trans| of this many votes, 1 .. 2^31 - 1 [2] */
	int32_t edges;        /* 1: an E line per edge */
	int32_t stats_only;   /* the header and the T line only */
	int32_t reserved;
	int64_t chunk_size;   /* bases per device chunk; a sequence is never cut [1 << 28] */
} yakamd_phopt_t;
void yakamd_phopt_init(yakamd_phopt_t *o);

yakamd_phase_t *yakamd_phase_open(int64_t n_bubble);
int     yakamd_phase_stats(yakamd_phase_t *ph, yakamd_phstat_t *st);
int     yakamd_phase_votes_dev(yakamd_phase_t *ph, const yakamd_aobs_t *d_obs, int64_t n_obs, int64_t n_out[2]);
int64_t yakamd_phase_pairs_dev(yakamd_phase_t *ph, void *d, int64_t cap);           /* n_pair entries of yakamd_ppair_t */
int     yakamd_phase_solve_dev(yakamd_phase_t *ph, const yakamd_asup_t *d_sup, int64_t n_sup, int32_t min_sup, int32_t min_link);
int64_t yakamd_phase_nodes_dev(yakamd_phase_t *ph, void *d, int64_t cap);           /* n_bubble entries of yakamd_pnode_t */
int64_t yakamd_phase_edges_dev(yakamd_phase_t *ph, void *d, int64_t cap);           /* n_edge entries of yakamd_pedge_t */
int64_t yakamd_phase_blocks_dev(yakamd_phase_t *ph, void *d, int64_t cap);          /* n_block entries of yakamd_pblock_t */
int     yakamd_phase_reset(yakamd_phase_t *ph);
void    yakamd_phase_close(yakamd_phase_t *ph);

/* `yak-amd bubbles -r -p` as a library call: what yakamd_alleles() opens -- the walk at min_cnt, the links, the bubbles, the arm map and the
 * index of the paths --, then the reads of reads_fn in chunks: upload, hits, chain, observations, votes; the records stay on the device.  Then
 * the support, the solve, the copies of the nodes, the blocks and (with edges) the edges and the pairs, and the text, tab-separated, which does
 * not depend on chunk_size:
 *   #phase k=<k> min_cnt=<c> min_sup=<m> min_link=<e>
 *   A ...                                        the A lines of `yak-amd bubbles -r`, byte for byte
 *   H <i> <block> <0|1>                          per het bubble, i ascending: the haplotype of allele 1
 *   K <block> <n_bubble> <n_edge> <n_disc> <w_sum> <w_disc>      per block of two or more, ascending
 *   E <i> <j> <cis> <trans> <forest|conc|disc>   with edges: per edge, sorted by (i, j) on the host
 *   T n_seq sum_len n_path n_step n_obs n_full n_vote n_pair n_bubble n_het n_edge n_forest n_disc n_block n_single max_block
 * max_block = the bubbles of the largest block, 1 where every het bubble stands alone.  With stats_only the header and the T line only.  0, or -1
 * after a message on stderr -- on a refusal before the output is created: everything yakamd_alleles() refuses, and min_link < 1 */
int     yakamd_phase(const yakamd_phopt_t *o, yak_ch_t *ch, const char *reads_fn, const char *out_fn);
/* measurement: the milliseconds the calling thread spent since its last yakamd_phase_open() on the compaction of the full records, the votes
 * with the growth of the table, the solve, the copies, the text */
void    yakamd_phase_ms(double ms[5]);
const char *yakamd_phase_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_allele_tally_names / _read / _reset are for libyak_amd_allele.so's */
int  yakamd_phase_tally_names(const char *const **names);
void yakamd_phase_tally_read(uint64_t *out, int n);
void yakamd_phase_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
