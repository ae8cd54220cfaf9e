/* yak_amd_path.h -- sequences laid onto the unitig graph of a count table as paths, on the GPU (libyak_amd_path.so; not in the reference; DESIGN.md
 * section 23).
 *
 * A layer above libyak_amd_walk.so and libyak_amd.so, built as libyak_amd_gfa.so is: it consumes the descriptors and the bases of a device walk
 * (include/yak_amd_walk.h) and seq_nt4_table, nothing else.  Node, unitig j, its bases S_j, n_node, open unitig, cycle,
 * (j, +) = S_j and (j, -) = revcomp(S_j) are those of yak_amd.h, yak_amd_walk.h and yak_amd_gfa.h; k is odd and in [3, 31].
 *
 * The index holds every node of every unitig: for unitig j and p in [0, n_node_j) let N = S_j[p : p + k]; the key is canon(N), the value
 * j << 32 | p << 1 | rev with rev = 1 iff N != canon(N).  Every node lies in one unitig once, so the keys are distinct.  A walk of 2^31 unitigs or
 * more, or with a unitig of 2^31 nodes or more, is refused.
 *
 * The hit array of a base image (what yakamd_lookup_dev() takes: 16-byte aligned, each sequence followed by '\n'; a byte is a base iff
 * seq_nt4_table[byte] < 4): Q_i is the k-mer ending at byte i, as read; it exists iff bytes i - k + 1 .. i are all bases.  hit[i] is
 * YAKAMD_PATH_NONE where no k-mer ends, YAKAMD_PATH_ABSENT where canon(Q_i) is no node, otherwise j << 32 | p << 1 | o with
 * o = (Q_i != canon(Q_i)) ^ rev: o = 0, the sequence passes the node as S_j does; o = 1, reverse-complemented.
 *
 * Position i is a hit iff hit[i] names a node.  i continues i - 1 iff both are hits with the same j and o and p_i = p_{i-1} + 1 for o = 0,
 * p_{i-1} - 1 for o = 1.  A step is a maximal run of positions each continuing the one before, written j << 1 | o; a path is a maximal run of
 * consecutive hits and consists of its steps in order.  Any non-base ends every k-mer across it: no path crosses a sequence boundary.  A wrap around
 * a cycle (p = n - 1 -> 0 for +, 0 -> n - 1 for -) does not continue: it starts a new step of the same unitig.  For consecutive steps a, b of a
 * path (a, b) is a link of yak_amd_gfa.h; only the first step of a path may begin inside its oriented unitig and only the last may end inside it.
 *
 * A path record: seq = the sequence's index among d_seq_off; [qs, qe) the bases of the sequence that the path covers
 * (qs = i_first - k + 1 - off[seq], qe = i_last + 1 - off[seq]); ps = the offset of the path's first base in its first oriented unitig (p_first for
 * o = 0, n_node - 1 - p_first for o = 1); its steps are steps[step_off .. step_off + n_step).  Both lists are in image order.  A tally per sequence:
 * its k-mers, its hits, its paths and its steps.
 *
 * yakamd_path_open(): copies of the walk's descriptors and bases are taken (the walk is not needed afterwards) and every node goes into a hash table
 * in device memory, which stays there until yakamd_path_close().  The device current at the call is used and stays current, here and in every call
 * below; all device pointers are the caller's.  NULL after a message (yakamd_path_last_error()), before any device work: w is NULL; k is even or
 * outside [3, 31]; k does not fit the walk; the walk is over the bounds above; the index needs more device memory than is free, or than
 * YAKAMD_PATH_MAX_BYTES, a test switch read from the environment -- 16 bytes a slot, the capacity a power of two at least twice n_node, plus the
 * copies of desc and bases; the message names the bytes.  YAKAMD_PATH_SLOTS, a test switch too, sets the capacity (rounded up to a power of two); a
 * value below n_node is refused.  A walk without unitigs opens, and every k-mer is absent.
 * stats: table_slots = the capacity; max_probe = the longest run of slots a claim or a look-up has inspected so far -- a measurement that may differ
 * between two calls; no result does.
 * yakamd_path_hits_dev(): d_hit (16-byte aligned, as d_bases) gets the entries [0, n_bytes rounded up to 16), NONE behind n_bytes; the image is read
 * up to the same bound.  0, or -1 after a message.
 * yakamd_path_chain_dev(): always writes n_out = { n_path, n_step } and, with n_seq > 0 and a d_tally, the tally of every sequence; the records only if
 * d_paths and d_steps are given and both caps (in entries) suffice.  0 when the records are written, 1 when it has only counted, -1 after a message.
 * d_paths and d_tally are 16-byte aligned, d_hit is as yakamd_path_hits_dev() wrote it, and an image of n_bytes > 0 has at least one sequence (a
 * path record names it).  With n_bytes = 0 it launches nothing. */
#ifndef YAK_AMD_PATH_H
#define YAK_AMD_PATH_H
#include "yak_amd_walk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YAKAMD_PATH_NONE   (~(uint64_t)0)
#define YAKAMD_PATH_ABSENT (~(uint64_t)0 - 1)

typedef struct yakamd_path yakamd_path_t;
typedef struct { uint64_t step_off, ps; uint32_t seq, n_step, qs, qe; } yakamd_upath_t;
typedef struct { uint32_t n_kmer, n_hit, n_path, n_step; } yakamd_ptally_t;
typedef struct { uint64_t n_unitig, n_node, table_slots, max_probe; } yakamd_pxstat_t;
typedef struct {
	int32_t min_cnt;      /* a k-mer with a count below this is absent, 1 .. 1023 [1] */
	int32_t min_len;      /* a path is written iff qe - qs >= min_len; a path covers k bases or more, so 0 keeps them all [0] */
	int32_t stats_only;   /* the tallies per sequence, not the paths */
	int32_t reserved;
	int64_t chunk_size;   /* bases per device chunk; a sequence is never cut [1 << 28] */
} yakamd_ppopt_t;
void yakamd_ppopt_init(yakamd_ppopt_t *o);

yakamd_path_t *yakamd_path_open(yakamd_uwalk_t *w, int k);        /* borrows w; index and a copy of desc stay on the device until close */
int     yakamd_path_stats(yakamd_path_t *px, yakamd_pxstat_t *st);
int     yakamd_path_hits_dev(yakamd_path_t *px, const void *d_bases, int64_t n_bytes, uint64_t *d_hit);
int     yakamd_path_chain_dev(yakamd_path_t *px, const uint64_t *d_hit, int64_t n_bytes,
                              const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                              yakamd_upath_t *d_paths, int64_t cap_paths, uint64_t *d_steps, int64_t cap_steps,
                              yakamd_ptally_t *d_tally, int64_t n_out[2]);
void    yakamd_path_close(yakamd_path_t *px);

/* `yak-amd paths` as a library call: the walk at min_cnt, the index, the walk closed, then the sequences of fn (FASTA or FASTQ, plain or gzip, `-`
 * for stdin) in chunks.  The text, tab-separated: one GAF line per path with qe - qs >= min_len, in input order,
 *   name  len  qs  qe  +  <path>  plen  ps  pe  nm  nm  255
 * <path> `>u<j>` or `<u<j>` per step (the names of the S lines of `unitigs -G`), plen the sum of the steps' n_node plus k - 1, pe = ps + qe - qs,
 * nm = qe - qs; with stats_only `#paths k=<k> min_cnt=<c>`, a line `S name len n_kmer n_hit n_path n_step` per sequence and
 * `T n_seq sum_len sum_kmer sum_hit sum_path sum_step` last.  The text does not depend on chunk_size.  0, or -1 after a message on stderr -- on a
 * refusal before the output is created: everything yakamd_uwalk_open() and yakamd_path_open() refuse, a table marked homopolymer-compressed, an
 * input that cannot be opened, min_len < 0, chunk_size < 1 */
int     yakamd_paths(const yakamd_ppopt_t *o, yak_ch_t *ch, const char *fn, const char *out_fn);
/* measurement: the milliseconds the calling thread's last yakamd_path_open / yakamd_paths call spent on the index and, summed over the chunks, on
 * the hits, the count and the scan, the emit, the copies, the text; yakamd_path_open() sets all six back, and every later yakamd_path_hits_dev() and
 * yakamd_path_chain_dev() of the thread adds to its part */
void    yakamd_path_ms(double ms[6]);
const char *yakamd_path_last_error(void);

/* the launch tally of this library's own kernels, as yakamd_gfa_tally_names / _read / _reset are for libyak_amd_gfa.so's */
int  yakamd_path_tally_names(const char *const **names);
void yakamd_path_tally_read(uint64_t *out, int n);
void yakamd_path_tally_reset(void);

#ifdef __cplusplus
}
#endif
#endif
