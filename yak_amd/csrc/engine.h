/* engine.h -- internal interface between pool.cpp, the engine (engine_ctx.cpp, engine_pass.cpp, engine_acc.cpp, engine_count.cpp, engine_slice.cpp, engine_table.cpp), table_read.cpp,
 * lookup_dev.cpp and the yak.h surface (yak_api.cpp, yak_table_ops.cpp, yak_file.cpp, yak_count.cpp, yak_reader.cpp, yak_multi.cpp, yak_inspect.cpp, yak_print.cpp) */
#ifndef YK_ENGINE_H
#define YK_ENGINE_H
#include <vector>
#include "../../include/yak_amd.h"
#include "yk_device.h"
#include "table_ranges.h"

/* what a command or export says of a table it cannot read as one image (yak_api.cpp multi_refuse, table_read.cpp yk_image_state) */
#define YK_MSG_SHARDED "not available on a table sharded over prefix ranges"

/* a device buffer kept from one chunk, batch or call to the next and grown when one needs more (yakamd_dev_alloc / yakamd_dev_free are hipMalloc /
 * hipFree).  An instance that lives until the process ends is held through a pointer that is never deleted: its destructor must not run after
 * the HIP runtime has shut down */
struct GrowBuf {
	void *p = 0;
	size_t cap = 0;
	GrowBuf() = default;
	GrowBuf(const GrowBuf&) = delete;
	GrowBuf &operator=(const GrowBuf&) = delete;
	~GrowBuf() { drop(); }
	bool fit(size_t n) { if (n <= cap) return true; drop(); p = yakamd_dev_alloc(n + n / 8); if (p) cap = n + n / 8; return p != 0; }
	void drop() { yakamd_dev_free(p); p = 0; cap = 0; }
};

struct yak_ht_t;
yakamd_ctx *yk_ctx_create(int k, int pre, int n_hash, int n_shift);
void yk_ctx_next_device(int dev);
void yk_ctx_destroy(yakamd_ctx *c);
int  yk_ctx_destroy_bf(yakamd_ctx *c);
int  yk_ctx_clear(yakamd_ctx *c);
int  yk_ctx_hist(yakamd_ctx *c, int64_t *cnt1024);
int  yk_ctx_setcnt(yakamd_ctx *c, int cnt);
int  yk_ctx_shrink(yakamd_ctx *c, int cmin, int cmax, u64 *tot);
int  yk_ctx_subtract(yakamd_ctx *c, yakamd_ctx *other, u64 *tot);
int  yk_ctx_isec(yakamd_ctx *c, yakamd_ctx *other, u64 *tot);
int  yk_ctx_tighten(yakamd_ctx *c);
int  yk_ctx_merge_presize(yakamd_ctx *c, yakamd_ctx *other);
int  yk_ctx_list_hashes(yakamd_ctx *c, int cmin, int cmax, u64 **d_hash, u32 **d_t, u64 *n, unsigned short **d_cnt = 0);   /* d_cnt: the listed keys' counts too */
int  yk_ctx_add_counts(yakamd_ctx *c, const u64 *d_hash, const unsigned short *d_cnt, u64 n);   /* the count step of yakamd_ch_sum; not inside a pass */
int  yk_ctx_in_pass(yakamd_ctx *c);
void yk_pool_release(void *p);
int yk_set_error(const char *fmt, ...);                      /* this thread's yakamd_last_error() text (+ a line on stderr); returns -1 */
void *yk_pool_get(size_t bytes);
void *yk_pool_alloc(size_t bytes, bool plain);              /* pool.cpp: a device buffer from the current device's pool (plain: never from the virtual-memory tier); 0 when the device is full */
void yk_pool_free(void *p);
double yk_now_ms(void);                                      /* monotonic wall clock */
int yk_ctx_dump_image_dev(yakamd_ctx *c, int lo, int hi, u64 **d_img, u64 *n_words);   /* the .yak bytes of sub-tables [lo, hi), in pool memory: StagedRange's to call */

/* ---- table_read.cpp: what the commands that read a resident table's stored keys share ---- */
/* a run of sub-tables [lo, hi) that one shard of a table owns, and that shard's context */
struct TablePiece { yakamd_ctx *c; int lo, hi; };
/* [lo, hi) of `h` cut by owner, in prefix order (a yakamd_set_shard table: the part of [lo, hi) it owns); false after a message that starts with
 * `what`: not an engine table, a range outside the table, a shard in an open pass */
bool yk_table_pieces(const yak_ch_t *h, int lo, int hi, const char *what, std::vector<TablePiece> *out);
/* the range rule (table_ranges.h) over the sizes of sub-tables [lo, hi) of one context */
std::vector<TableRange> yk_ctx_ranges(yakamd_ctx *c, int lo, int hi, int64_t budget, bool keep_empty);
/* the owner of one staged range: the .yak body of sub-tables [lo, hi) of a context (pool memory of its device; per sub-table the {capacity, size}
 * word, then the stored keys in ascending slot order) and, when asked for, the device copy of the range's key offsets, in a buffer kept from one
 * range to the next.  One owner serves the contexts of one call; whatever it holds goes back with the context's device selected */
struct StagedRange {
	u64 *d_img = 0;
	u64 n_words = 0;
	GrowBuf d_off;                                               /* (which makes the owner one that is not copied) */
	~StagedRange() { drop(); }
	/* the image of [lo, hi) in place of the one held; off != 0: those offsets (hi - lo + 1 of them) beside it, after the check that the image holds
	 * off->back() keys -- else "<what>: the table changed while it was <verb>".  0, or -1 after a message */
	int stage(yakamd_ctx *c, int lo, int hi, const std::vector<u64> *off = 0, const char *what = 0, const char *verb = 0);
	void drop();                                                 /* the image goes back to the pool; the offsets' buffer stays */
	const u64 *off() const { return (const u64*)d_off.p; }
private:
	int dev = -1;
};
void yk_ctx_gate(yakamd_ctx *c, bool on);
void yk_ctx_or_mode(yakamd_ctx *c, int mode);   /* 0 counting; 1 flag loads; 2 saved-count loads (yk_device.h FastParams.or_mode) */
void yk_ctx_lock(yakamd_ctx *c);
void yk_ctx_unlock(yakamd_ctx *c);
void *yk_ctx_scratch(yakamd_ctx *c, size_t bytes);
int  yk_ctx_inc(yakamd_ctx *c, u64 hash, int *count);
int  yk_ctx_resize_to(yakamd_ctx *c, const uint32_t *want);
u64  yk_ctx_keys_total(yakamd_ctx *c);
void yk_ctx_range(yakamd_ctx *c, int *lo, int *hi);   /* the prefix range [lo, hi) this context owns (yakamd_set_shard) */
int  yk_ctx_load(yakamd_ctx *c, const uint32_t *caps, const uint32_t *sizes, const uint64_t *keys);
int  yk_ctx_sync_host(yakamd_ctx *c, yak_ch_t *h);
u64  yk_ctx_list_time(yakamd_ctx *c, u64 n);
int  yk_ctx_device(yakamd_ctx *c);
int  yk_inspect_engines(const yak_ch_t *h, std::vector<yakamd_ctx*> *eng);   /* the engines of a table (one per rank of a sharded one), all on one device and out of a pass */
/* lookup_dev.cpp, `yak-amd depth`: windows [g0, g0 + n_win) of a call as yakamd_depth_reduce_dev() takes it into d_win[0 .. n_win) (24 bytes each),
 * n_win at most yk_depth_batch_max() (2^24; the test switch YAKAMD_DEPTH_BATCH lowers it); the caller synchronises `st` */
int64_t yk_depth_batch_max(void);
int  yk_depth_batch(int k, int64_t w, const void *d_cnt_u16, const uint64_t *d_seq_off, const uint32_t *d_seq_len, const uint64_t *d_win_off,
                    int64_t n_seq, int64_t n_bytes, uint64_t g0, uint32_t n_win, void *d_win, hipStream_t st);
/* yak_hpc.cpp: homopolymer compression (kern_hpc.inc) of an ASCII (valid == 0) or packed image on `st` into `out` (room for n rounded up to 16), with
 * n_seq > 0 the sequences' offsets and lengths in the compressed image too; returns the compressed length, or -1 after a message.  Synchronises `st` */
int64_t yk_hpc_compact(const void *in, const u32 *valid, int64_t n, void *out, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                       uint64_t *d_seq_off_out, uint32_t *d_seq_len_out, hipStream_t st);
size_t yk_pool_cached_bytes(void);
size_t yk_pool_held_bytes(int dev);
void yk_pool_report(const char *what);
hipStream_t yk_ctx_stream(yakamd_ctx *c);
void yk_ctx_set_source(yakamd_ctx *c, const uint64_t id[4], int64_t n_seq);
bool yk_ctx_same_source(yakamd_ctx *c, const uint64_t id[4], int64_t *n_seq);
#endif
