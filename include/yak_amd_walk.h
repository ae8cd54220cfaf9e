/* yak_amd_walk.h -- the unitigs of a count table's de Bruijn graph walked on the GPU (libyak_amd_walk.so; not in the reference).
 *
 * A layer above libyak_amd.so: it consumes the records of yakamd_graph_nodes_dev() (include/yak_amd.h) and ranks the 2 n_key
 * traversal states of the table by pointer doubling over their links.  All definitions -- node, listing index, side, link, traversal state (v, d),
 * unitig, order and orientation -- are those of yak_amd.h; yakamd_unitigs() and its host walk are untouched and give the same text.
 *
 * Let j number the unitigs in output order from 0: the open ones ascending by the listing index of their start node, then the cycles ascending by
 * their smallest index.  Unitig j of n nodes visits the states (v_0, d_0) .. (v_{n-1}, d_{n-1}): an open unitig from its start node, read away from
 * its unlinked side (a node without a link as stored), a cycle from its smallest node as stored through R.  Three arrays stay in device memory
 * until yakamd_uwalk_close():
 *   map     per stored key in listing order: the unitig j it lies in and p << 1 | d_p for its place v_p; YAKAMD_GRAPH_NONE, 0 for a key that is no node
 *   desc    per unitig: its n_node + k - 1 bases start at bases[off]; kc = the sum of its nodes' counts; first = v_0 << 1 | (1 for a cycle)
 *   bases   ASCII ACGT, the unitigs back to back in order j; off is the exclusive scan of n_node + k - 1
 * The bases of a unitig are the k bases of v_0 as read in d_0 and, for p >= 1, the last base of v_p as read.
 *
 * yakamd_uwalk_open(): the graph is opened, all records go to device memory in one yakamd_graph_nodes_dev(0, 1 << pre) call, the graph is closed,
 * the walk runs.  NULL after a message (yakamd_walk_last_error()), before any device work of the walk: everything yakamd_graph_open() refuses, with
 * its message; and a walk that needs more device memory than is free (or than YAKAMD_WALK_MAX_BYTES, a test switch read from the environment) --
 * about 136 bytes per stored key while it runs, the message names the bytes.
 * The three _dev getters copy into device memory of the caller (cap in entries; map and desc 16-byte aligned) and return the number of entries; with
 * a NULL pointer or a smaller cap the number needed, and nothing is written.  -1 after a message.
 * yakamd_uwalk_open() leaves the table's device current, as yakamd_graph_open() does; the getters and the close work on that device and make the
 * caller's current again.
 * stats: rounds = the doubling rounds run; host_nodes = the records whose contents reached the host during the walk: those of the nodes on cycles,
 * never one of an open unitig. */
#ifndef YAK_AMD_WALK_H
#define YAK_AMD_WALK_H
#include "yak_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yakamd_uwalk yakamd_uwalk_t;
typedef struct { uint64_t unitig, at; } yakamd_umap_t;
typedef struct { uint64_t off, n_node, kc, first; } yakamd_udesc_t;
typedef struct { uint64_t n_key, n_node, n_open, n_cycle, sum_len, max_len, n50, rounds, host_nodes; } yakamd_uwstat_t;

yakamd_uwalk_t *yakamd_uwalk_open(yak_ch_t *h, int min_cnt);
int     yakamd_uwalk_stats(yakamd_uwalk_t *w, yakamd_uwstat_t *st);
int     yakamd_uwalk_gstat(yakamd_uwalk_t *w, yakamd_gstat_t *st);          /* the graph's tallies taken at open, for the -s text */
int64_t yakamd_uwalk_map_dev  (yakamd_uwalk_t *w, void *d, int64_t cap);    /* n_key entries */
int64_t yakamd_uwalk_desc_dev (yakamd_uwalk_t *w, void *d, int64_t cap);    /* n_open + n_cycle entries */
int64_t yakamd_uwalk_bases_dev(yakamd_uwalk_t *w, void *d, int64_t cap);    /* sum_len bytes */
void    yakamd_uwalk_close(yakamd_uwalk_t *w);

/* `yak-amd unitigs -g` as a library call: byte for byte the text of yakamd_unitigs(), FASTA or with stats_only the tallies, made on the host from
 * the descriptors and the bases; n_threads and batch_keys of the options are ignored.  0, or -1 after a message on stderr -- on a refusal before the
 * output is created */
int     yakamd_unitigs_dev(const yakamd_ugopt_t *o, yak_ch_t *ch, const char *out_fn);
/* measurement: the milliseconds the calling thread's last yakamd_uwalk_open / yakamd_unitigs_dev call spent on the graph, the records, the ranking
 * rounds, the numbering and the bases (cycles included), the copies out, the text */
void    yakamd_uwalk_ms(double ms[6]);
const char *yakamd_walk_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_tally_names / _read / _reset are for libyak_amd.so's */
int  yakamd_walk_tally_names(const char *const **names);
void yakamd_walk_tally_read(uint64_t *out, int n);
void yakamd_walk_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
