/* engine_int.h -- what the engine's own translation units (engine_ctx.cpp: the context; engine_pass.cpp: passes and feeds; engine_acc.cpp: the
 * accumulator path of a create pass; engine_count.cpp: counting into existing keys, by the plan of count_plan.h; engine_slice.cpp: the count of a slice; engine_table.cpp: whole-table operations; layout.cpp: exact slot layout; table_read.cpp: the staged ranges, owner cut and
 * refusals of the commands that read a table's stored keys; lookup_dev.cpp: the device-level exports of the lookup commands; yak_hetmer.cpp and
 * yak_graph.cpp: hetmers and unitigs) share and nobody else sees: the context of a table with the buffers it owns (dev_buf.h), the error macro, and the few functions that
 * cross between those files. */
#ifndef YK_ENGINE_INT_H
#define YK_ENGINE_INT_H
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <vector>
#include <map>
#include <string>
#include <mutex>
#include <atomic>
#include <algorithm>
#include <memory>
#include "yk_device.h"
#include "tally.h"
#include "engine.h"
#include "dev_buf.h"

#define fail(...) yk_set_error(__VA_ARGS__)                  /* this thread's yakamd_last_error() text + a line on stderr; -1 */
#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail("%s:%d: %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); } while (0)

static inline double now_ms() { return yk_now_ms(); }

static inline int64_t env_i64(const char *name, int64_t dflt) { return yk_knob(name, dflt); }

static inline int ceil_log2_u64(u64 x) { int b = 0; while ((1ull << b) < x) ++b; return b; }

/* khashl resize target (reference khashl.h:155-158): bits for a requested slot count */
static inline u32 kh_bits_for(u32 want)
{
	u32 lg = 0, x = want;
	while ((x >>= 1) != 0) ++lg;
	if (want & (want - 1)) ++lg;
	return lg > 2 ? lg : 2;
}

/* engine_ctx.cpp: streams and events are kept and handed out again (creating one costs a runtime call) */
hipStream_t yk_stream_get(int dev);
void yk_stream_put(int dev, hipStream_t x);
hipEvent_t yk_ev_get();
void yk_ev_put(hipEvent_t e);

struct EvTimer {
	hipEvent_t a, b; hipStream_t st;
	EvTimer(hipStream_t s) : st(s) { a = yk_ev_get(); b = yk_ev_get(); hipEventRecord(a, st); }
	double stop() { float ms = 0; hipEventRecord(b, st); hipEventSynchronize(b); hipEventElapsedTime(&ms, a, b); return ms; }
	~EvTimer() { yk_ev_put(a); yk_ev_put(b); }
};

/* the stream of a context, handed back to the cache when the context goes */
struct CtxStream {
	hipStream_t s = 0; int dev = 0;
	operator hipStream_t() const { return s; }
	~CtxStream() { if (s) yk_stream_put(dev, s); }
};
struct HostFree { void operator()(void *p) const { (void)hipHostFree(p); } };
struct CFree { void operator()(void *p) const { free(p); } };
struct yak_ht_t;

/* fast path: a level-1 partitioned batch kept until the slice is counted.  d_rec views the records, YK_FMT_POS or YK_FMT_TAGGED: the batch's own buffer, or the caller's */
struct Kept { DevBuf<Rec> own; const void *d_rec = 0; RecFmt fmt = YK_FMT_POS; u64 n = 0; u64 t0 = 0, span = 0; std::vector<u64> bstart; };

/* what a pass holds and pass_free gives back */
struct PassBufs {
	std::vector<Kept> kept; u64 kept_bytes = 0;
	AccTab acc = {}; DevBuf<AccSlot> acc_mem; u64 acc_count = 0;   /* the accumulator as the kernels see it, and its storage */
	DevVec<Rec> rec;
	DevVec<uint8_t> hpc;               /* a table in homopolymer-compressed space compacts every feed of bases into this buffer */
	DevVec<u64> newlist, miss, cand;   /* the bloom gate's lists, grown together (new_reserve) */
};

/* level-1 records of the last create_new pass, kept for a count pass over the SAME input (yakamd_retain_input / yakamd_count_retained):
 * the second pass of the bloom protocol (reference main.c:53-57) then neither reads nor hashes the input again */
struct Retained { DevBuf<Rec> rec; u64 n = 0; std::vector<u64> bstart; };
/* ... or, when the whole pass was one slice into an empty table, its level-2 records (grouped by sub-bucket) + the keys every sub-bucket put
 * into the table: the count pass then owns each key's counter in LDS (k_cnt2) -- or, with kc2, takes every key's count as k_lc2 found it
 * (the same records: min(instances, 1023) per key, in kkc's order) and only applies them */
struct Ret2 {
	DevBuf<Rec> r2; DevBuf<u64> sbstart, koff, kkc, segbase; DevBuf<u32> kc2; FastParams fp = {}; u64 n_total = 0, n_keys = 0; bool valid = false;
	/* kkc lists every key of the image exactly once, each with the count the image holds for it (fast_finish: the pass began on an empty image, ended
	 * in one slice and kept kc2), and nothing has touched keys or counts since -- yak_ch_clear apart (yk_image_touched) */
	bool whole_image = false;
};
/* what retained_drop gives back */
struct RetainedInput { std::vector<Retained> l1; u64 l1_bytes = 0; Ret2 l2; };

struct yakamd_ctx {
	CtxStream st;                      /* declared first, so handed back last: behind the frees of every buffer below */
	int k = 0, pre = 0, P = 0, n_hash = 0, bf_shift = 0, nb = 0;
	bool has_bloom = false;
	int dev = 0, plo = 0, phi = 0;

	/* table image */
	DevBuf<u32> d_bits, d_used, d_delta;
	DevBuf<u64> d_off, d_keys;
	u64 n_slots = 0;                   /* arena size (multiple of 32) */
	std::vector<u32> h_bits, h_count;
	std::vector<u64> h_off;
	u64 img_keys_total = 0;            /* sum of counts */
	std::atomic<bool> clear_pending{false};   /* yak_ch_clear was asked for and k_img_clear has not run yet: the next reader or writer of the image launches it (img_view; readers may be several threads) */

	/* bloom */
	DevBuf<u32> d_bf; size_t bf_words = 0;
	bool bf_virgin = false;            /* allocated but never written: logically all zero */
	bool bf_deferred = false;          /* the last pass left its bits in LDS only (FastParams.bf_nowb): the filter is whatever k_bf_rebuild makes of the retained records (ret.l2) */
	DevBuf<u32> d_multi; int multi_bits = 0;

	/* running pass */
	bool delta_dirty = false;          /* the running pass left pending counts in d_delta (k_img_fold at its end) */
	bool in_pass = false; int create_new = 0; bool bloom_mode = false; bool gate_off = false; int or_mode = 0;   /* gate_off: puts of a merge never consult the filter */
	PassBufs pass;
	DevBuf<u64> d_counters, d_lastput, d_lpbatch;
	DevBuf<u32> d_missing, d_nmissing;
	DevVec<uint8_t> stage;             /* the staging buffer of the host feeds */
	bool hpc = false;                  /* the table lives in homopolymer-compressed space (yakamd_ch_set_hpc): every feed of bases is compacted first */
	DevVec<u32> rows; DevBuf<u64> d_partial, d_bstart; int nb_bits = 0;   /* the level-1 partition's scratch; rows holds NB x blocks */
	bool fast = false; u64 fast_budget = 0; u64 t_pass0 = 0; bool t_pass0_set = false; u64 keys_at_begin = 0;
	double ms_part2 = 0, ms_lds = 0;
	u64 t_end = 0;
	u64 list_t = 0;                    /* running stream time of yak_ch_insert_list calls */
	yakamd_stats_t st_cur = {}, st_last = {};

	RetainedInput ret; bool retain_on = false, retain_broken = false;
	int n_slices = 0;                  /* slices of the running pass counted so far (fast_flush_slice) */
	u64 src_id[5] = {}; bool src_set = false;   /* identity of the file the retained records came from + its sequence count (yak_count) */

	std::mutex api_mu;                 /* serialises whole-table entry points that callers may reach from several threads (yak_ch_insert_list) */
	DevVec<uint8_t> scratch;

	/* host mirror */
	bool host_valid = false;
	std::unique_ptr<u64[], HostFree> hm_keys; std::unique_ptr<u32[], HostFree> hm_used; u64 hm_slots = 0;
	std::unique_ptr<yak_ht_t[], CFree> hts;
};

struct yak_ch_ext { yak_ch_t pub; yakamd_ctx *ctx; u32 magic; int n_sub; yak_ch_t **sub; };   /* n_sub > 1: a table sharded over several GPUs (yak_api.cpp) */
#define EXT_MAGIC 0x59414b41u

static inline yakamd_ctx *ctx_of(const yak_ch_t *h)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	return (h && e->magic == EXT_MAGIC) ? e->ctx : 0;
}

/* engine_table.cpp: a pending yak_ch_clear becomes real (k_img_clear on the table's stream, waited for).  Whatever reads or writes the image's keys goes
 * through here first: img_view below, and the few places that take c->d_keys themselves (layout.cpp, the host mirror, the khashl resizes) */
int yk_image_settle(yakamd_ctx *c);
/* keys or counts of the image change by something other than yak_ch_clear: the retained key list no longer stands for the image */
static inline void yk_image_touched(yakamd_ctx *c) { c->ret.l2.whole_image = false; }

/* the image as it is, a pending clear left pending: for the one caller that folds the clear into its own sweep (yakamd_count_retained) */
static inline ImgView img_view_pending(yakamd_ctx *c)
{
	ImgView v;
	v.bits = c->d_bits; v.off = c->d_off; v.keys = c->d_keys; v.used = c->d_used; v.delta = c->d_delta;
	v.pre = c->pre; v.k = c->k;
	return v;
}
static inline ImgView img_view(yakamd_ctx *c)
{
	if (c->clear_pending) (void)yk_image_settle(c);          /* (a launch that fails shows in the caller's own checks of the stream) */
	return img_view_pending(c);
}

/* table_read.cpp: how a table stands to a command that reads it as one image.  c: its context, the first shard's of a table spread over several
 * GPUs (which has none of its own), 0 if `h` is no engine table; sharded: it cannot be read as one image -- several GPUs' tables, or a
 * yakamd_set_shard range; in_pass: a shard of it is in an open pass */
struct ImageState { yakamd_ctx *c; bool sharded, in_pass; };
ImageState yk_image_state(const yak_ch_t *h);
/* the context a command that probes the whole image of a table of odd k < 32 for its keys at min_cnt or above works on (hetmers, the graph), or 0
 * after fail(): every refusal, in the order of include/yak_amd.h, before any device work.  no_gpu / even_k: the command's own ends of those two texts */
yakamd_ctx *yk_whole_image_ctx(const yak_ch_t *h, int min_cnt, const char *what, const char *no_gpu, const char *even_k);

/* the text a command writes: to `fn`, or to stdout for NULL and "-".  A file is closed when the owner goes; finish() tells whether all of it got out */
struct OutFile {
	FILE *f = 0;
	const char *name = "-";
	bool own = false;
	OutFile() = default;
	OutFile(const OutFile&) = delete;
	OutFile &operator=(const OutFile&) = delete;
	~OutFile() { if (own && f) fclose(f); }
	bool open(const char *fn) { own = fn && strcmp(fn, "-") != 0; if (own) name = fn; f = own ? fopen(fn, "wb") : stdout; return f != 0; }
	bool finish() { bool ok = fflush(f) == 0 && !ferror(f); if (own) { ok = fclose(f) == 0 && ok; f = 0; } return ok; }
};

/* layout.cpp: the exact khashl slot layout (khashl.h:152-221) of `m[p]` new keys per sub-table, sorted by insertion time, on top of the table image */
int yk_run_replay(yakamd_ctx *c, const std::vector<u32> &m, const u64 *d_rec_kc, const u64 *d_rec_t,
                  const u64 *d_lastput, const std::vector<u32> *init_bits, bool from_empty, const std::vector<u64> *rec_off = 0);
/* layout.cpp: the new image replaces the context's -- `keys` / `used`, an arena of tot slots, sub-table p at new_off[p] with c->h_bits[p] / c->h_count[p] */
int yk_image_commit(yakamd_ctx *c, DevBuf<u64> &&keys, DevBuf<u32> &&used, u64 tot, const std::vector<u64> &new_off);
void yk_replay_counters(u32 *used, u32 *refused);            /* debug: replays done by the streaming kernels / handed back to k_replay */

/* a chunk table of the level-2 partition kernels: work items of at most a given number of records, each inside one bucket, grouped by bucket
 * (first[q]: bucket q's first item, first[n_buckets]: their number); the last item of a bucket has spare = 1 */
struct ChunkTable {
	std::vector<Chunk2> h;
	std::vector<u32> first;
	DevBuf<Chunk2> d; DevBuf<u32> d_first;
	int upload(hipStream_t st)                                   /* (the host tables must outlive the copies: the caller synchronises) */
	{
		if (d.alloc(h.size()) || d_first.alloc(first.size())) return -1;
		HIPCK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(Chunk2), hipMemcpyHostToDevice, st));
		HIPCK(hipMemcpyAsync(d_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, st));
		return 0;
	}
	void reset() { d.reset(); d_first.reset(); }
};
/* engine_slice.cpp: the runs [start[q], start[q + 1]) of buckets q < n_buckets, records of `stride` bytes from `base`, cut into items of at most `len` records */
void chunk_runs(ChunkTable &t, const void *base, size_t stride, const u64 *start, size_t n_buckets, u64 len);

/* the time of an insert kernel (timed by tm) into the pass's statistics */
static inline double insert_ms(yakamd_ctx *c, EvTimer &tm) { const double ms = tm.stop(); c->st_cur.ms_insert += ms; c->st_cur.ms_dominant_kernel += ms; c->st_cur.n_dominant_launches += 1; return ms; }

/* engine_ctx.cpp */
BloomView bloom_view(yakamd_ctx *c);
int bloom_materialise(yakamd_ctx *c);                       /* give a never-written bloom array its zeros */
int delta_ensure(yakamd_ctx *c);                            /* the per-slot pending increments exist from here to the end of the pass */
void retained_drop(yakamd_ctx *c);
void pass_free(yakamd_ctx *c);
/* engine_pass.cpp: records [0, n_rec) of d_rec (times = t0 + position, all within [batch_lo, batch_hi)) -> table.  A create pass takes YK_FMT_POS alone.
 * d_bstart: the records are grouped by level-1 bucket, and these are the buckets' starts */
int consume_records(yakamd_ctx *c, const void *d_rec, RecFmt fmt, int64_t n_rec, u64 t0, u64 batch_lo, u64 batch_hi, const u64 *d_bstart = 0);
int part_reserve(yakamd_ctx *c, int n_blk);                 /* the level-1 partition's scratch (rows, d_partial, d_bstart): room for a launch of n_blk blocks */
/* engine_acc.cpp: the accumulator path of a create pass -- a batch into the accumulator; at the end of the pass its new keys into the image (*n_ins of them) */
int acc_records(yakamd_ctx *c, const Rec *rec, int64_t n_rec, u64 t0, u64 batch_lo, u64 batch_hi);
int acc_finish(yakamd_ctx *c, int64_t *n_ins);
/* engine_count.cpp: a batch counted into the keys the table holds, by the plan of count_plan.h; the format that plan wants a count pass's extraction to write */
int count_records(yakamd_ctx *c, const void *d_rec, RecFmt fmt, int64_t n_rec, const u64 *d_bstart);
RecFmt count_pass_fmt(const yakamd_ctx *c);
/* engine_slice.cpp: the exclusive-ownership path of a create pass.  fast_admit: *out = the admitted batch's own buffer (0 when the records are `borrowed`) */
int fast_admit(yakamd_ctx *c, RecFmt fmt, u64 t, u64 n_pos, u64 n_cap, void **out, const void *borrowed = 0);
int fast_keep(yakamd_ctx *c, u64 n_rec);
int fast_abandon(yakamd_ctx *c);
int fast_finish(yakamd_ctx *c, bool last = false);
#endif
