/* yak_amd_gfa.h -- the compacted de Bruijn graph of a count table as GFA 1: the links between its unitigs made on the GPU (libyak_amd_gfa.so; not in
 * the reference).
 *
 * A layer above libyak_amd_walk.so and libyak_amd.so: it consumes the descriptors and the bases of a device walk (include/yak_amd_walk.h, DESIGN.md
 * section 21) and nothing else.  All definitions -- node, unitig, its order j, its bases S_j, open unitig and cycle -- are those of yak_amd.h and
 * yak_amd_walk.h.
 *
 * An oriented unitig is (j, +) = S_j or (j, -) = revcomp(S_j).  For an open unitig and an orientation o let W be the last k bases of (j, o), and for
 * each base b in the order A, C, G, T let Z = W[1:] + b.  If canon(Z) is the first or the last node of an open unitig j', there is a link
 * (j, o) -> (j', o'): o' is + if the first k bases of S_j' equal Z, otherwise it is - and the first k bases of revcomp(S_j') equal Z (exactly one
 * holds: k is odd and the nodes of a unitig are distinct).  A cycle has exactly the two links (j, +) -> (j, +) and (j, -) -> (j, -).  An arc that is
 * not a link inside a unitig joins two unlinked end sides, so the end nodes of the open unitigs are all that has to be looked up.
 * The links are listed by j ascending, + before -, then by b; a link is (from, to), each unitig << 1 | (1 for '-').  With the graph's tallies
 * (yakamd_gstat_t): n_link = n_arc - n_linked_side + 2 n_cycle; the mirror (j', flip o') -> (j, flip o) of every link is in the list (a link that
 * is its own mirror once); an oriented end has at most 4 links.
 *
 * yakamd_gfa_open(): copies of the walk's descriptors and bases are taken (the walk is not needed afterwards), the end nodes go into a hash table
 * in device memory, every oriented end counts and then writes its links; the links stay in device memory until yakamd_gfa_close().  The work is
 * done on the device that is current at the call, which stays current.  NULL after a message (yakamd_gfa_last_error()), before any device work:
 * w is NULL; k is even or outside [3, 31]; k does not fit the walk (sum_len != n_node + (n_open + n_cycle) (k - 1)).  A walk without unitigs opens
 * and has no link.  YAKAMD_GFA_SLOTS, a test switch read from the environment, sets the capacity of the hash table (rounded up to a power of two);
 * a value below the number of keys is refused.
 * stats: end_deg[d] = the oriented ends of open unitigs with d links (they sum to 2 n_open); table_slots = the capacity of the hash table;
 * max_probe = the longest run of slots a claim or a look-up inspected -- a measurement that may differ between two calls, as the slot a key lands
 * in depends on the order of the claims; no result does.
 * yakamd_gfa_links_dev() copies into device memory of the caller (cap in entries, 16-byte aligned) and returns the number of links; with a NULL
 * pointer or a smaller cap the number needed, and nothing is written.  -1 after a message. */
#ifndef YAK_AMD_GFA_H
#define YAK_AMD_GFA_H
#include "yak_amd_walk.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yakamd_gfa yakamd_gfa_t;
typedef struct { uint64_t from, to; } yakamd_ulink_t;
typedef struct { uint64_t n_unitig, n_open, n_cycle, n_link, end_deg[5], table_slots, max_probe; } yakamd_gfastat_t;

yakamd_gfa_t *yakamd_gfa_open(yakamd_uwalk_t *w, int k);   /* borrows w; links stay in device memory until close */
int     yakamd_gfa_stats(yakamd_gfa_t *g, yakamd_gfastat_t *st);
int64_t yakamd_gfa_links_dev(yakamd_gfa_t *g, void *d, int64_t cap);       /* n_link entries */
void    yakamd_gfa_close(yakamd_gfa_t *g);

/* `yak-amd unitigs -G` as a library call: the device walk, the links, and the text made on the host -- GFA 1: `H VN:Z:1.0`, a segment line
 * `S u<j> <bases> LN:i: KC:i: km:f: cl:i:<0|1>` per unitig with the values of the FASTA header (cl in lower case: GFA reserves upper-case tags), a
 * line `L u<a> <+|-> u<b> <+|-> <k-1>M` per link in list order; with stats_only the text of yakamd_unitigs_dev() followed by the line
 * `G n_link end_deg[0] .. end_deg[4]`.  All fields are separated by tabs.  0, or -1 after a message on stderr -- on a refusal before the output is
 * created */
int     yakamd_unitigs_gfa(const yakamd_ugopt_t *o, yak_ch_t *ch, const char *out_fn);
/* measurement: the milliseconds the calling thread's last yakamd_gfa_open / yakamd_unitigs_gfa call spent on the end table (with the copies of the
 * walk's results), the count and the scan, the emit, the text (with the copies out) */
void    yakamd_gfa_ms(double ms[4]);
const char *yakamd_gfa_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_walk_tally_names / _read / _reset are for libyak_amd_walk.so's */
int  yakamd_gfa_tally_names(const char *const **names);
void yakamd_gfa_tally_read(uint64_t *out, int n);
void yakamd_gfa_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
