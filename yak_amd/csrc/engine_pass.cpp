/* engine_pass.cpp -- a counting pass of the engine: yakamd_pass_begin and yakamd_pass_end, every yakamd_feed_* and yakamd_partition_* entry
 * point, and consume_records, which hands a batch to the path that takes it: the accumulator path of a create pass (engine_acc.cpp) or the
 * count of existing keys (engine_count.cpp).  The exclusive-ownership path of a create pass, which keeps its batches and counts them as slices,
 * is in engine_slice.cpp. */
#include "engine_int.h"

extern "C" int yakamd_pass_begin(yak_ch_t *h, int create_new)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c) return fail("not an engine table");
	if (c->in_pass) return fail("pass already open");
	HIPCK(hipSetDevice(c->dev));
	(void)hipGetLastError();                                   /* whatever other users of the runtime left behind is not this pass's (see yakamd_pass_end) */
	c->create_new = create_new;
	c->delta_dirty = false;
	if (!create_new && delta_ensure(c)) return -1;
	if (create_new) { retained_drop(c); c->retain_broken = false; }
	c->n_slices = 0;
	c->bloom_mode = create_new && c->has_bloom && !c->gate_off;
	c->in_pass = true;
	c->t_end = 0;
	c->st_cur = {};
	HIPCK(hipMemsetAsync(c->d_counters, 0, YKC_N * 8, c->st));
	HIPCK(hipMemsetAsync(c->d_lastput, 0, c->P * 8, c->st));
	c->st_cur.ms_total = now_ms();
	/* exclusive-ownership LDS counting needs level-1 buckets == sub-tables and 2-bit k-mers */
	c->fast = create_new && env_i64("YAKAMD_FAST", 1) != 0 && c->nb_bits == c->pre && (!c->has_bloom || c->nb <= 42);
	c->pass.kept_bytes = 0; c->t_pass0_set = false; c->ms_part2 = c->ms_lds = 0; c->keys_at_begin = c->img_keys_total;
	if (c->fast) {
		size_t fr = 0, tot = 0;
		HIPCK(hipMemGetInfo(&fr, &tot));
		c->fast_budget = (u64)env_i64("YAKAMD_FAST_BUDGET", (int64_t)((fr + yk_pool_cached_bytes()) / 4));
	}
	return 0;
}

/* the level-1 partition's scratch: room for a launch of n_blk blocks */
int part_reserve(yakamd_ctx *c, int n_blk)
{
	const size_t NB = (size_t)1 << c->nb_bits;
	if (!c->d_partial && (c->d_partial.alloc(NB * yk_part_groups()) || c->d_bstart.alloc(NB + 1))) return -1;
	return c->rows.reserve(NB * (size_t)n_blk);
}

int consume_records(yakamd_ctx *c, const void *d_rec, RecFmt fmt, int64_t n_rec, u64 t0, u64 batch_lo, u64 batch_hi, const u64 *d_bstart)
{
	if (n_rec <= 0) return 0;
	c->st_cur.n_instances += n_rec;
	if (batch_hi > c->t_end) c->t_end = batch_hi;
	return c->create_new ? acc_records(c, (const Rec*)d_rec, n_rec, t0, batch_lo, batch_hi) : count_records(c, d_rec, fmt, n_rec, d_bstart);   /* a create pass: {hash, position} records */
}

/* a base image on the device (ASCII, or packed with d_valid) into the open pass, a batch at a time */
static int feed_image(yak_ch_t *h, const void *d_bases, const u32 *d_valid, int64_t n_bytes, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	if (c->k >= 64 || c->k < 1) return fail("k must be in [1, 63]");
	if (((uintptr_t)d_bases & 15) != 0) return fail("device base image must be 16-byte aligned");
	HIPCK(hipSetDevice(c->dev));
	if (c->hpc && n_bytes > 0) {
		/* a table in homopolymer-compressed space: the image is compacted, ASCII or packed, into the pass's buffer and the feed goes
		 * on with that.  t0 stays the feed's position in the uncompressed stream: a compressed position is no larger than the original one, so the
		 * feeds keep their order, and only the order of stream positions matters */
		DevVec<uint8_t> &hpc = c->pass.hpc;
		if ((size_t)n_bytes > hpc.cap() && hpc.reserve((size_t)(((n_bytes + (n_bytes >> 3) + 4096) + 15) & ~(int64_t)15))) return -1;
		const int64_t n_out = yk_hpc_compact(d_bases, d_valid, n_bytes, hpc, 0, 0, 0, 0, 0, c->st);
		if (n_out < 0) return -1;
		d_bases = hpc.get(); d_valid = 0; n_bytes = n_out;
	}
	int64_t batch = env_i64("YAKAMD_BATCH", (int64_t)1 << 31);
	batch = std::min<int64_t>((int64_t)1 << 31, std::max<int64_t>(4096, batch & ~(int64_t)4095));   /* run starts are 31-bit (tagged records: bit 31 is the toggle) */
	const RecFmt consumed = c->create_new ? YK_FMT_POS : count_pass_fmt(c);   /* of a batch that is consumed at once; a count pass: the plan of the count says (count_plan.h) */
	/* a kept batch: tagged 8-byte records (half the partition traffic) when the hash leaves room for the tag, (hash >> pre) < 2^52 */
	const RecFmt kept = yk_tagged_fits(c->k, c->pre) && c->nb_bits == c->pre && !c->or_mode ? YK_FMT_TAGGED : YK_FMT_POS;
	const int64_t bmax = std::min(batch, (n_bytes + 4095) & ~(int64_t)4095);
	if ((!c->fast && c->pass.rec.reserve((size_t)bmax)) || part_reserve(c, yk_xpart_blocks(bmax))) return -1;   /* the fast path keeps every batch in a buffer of its own */
	for (int64_t pos = 0; pos < n_bytes; pos += batch) {
		const int64_t end = std::min(n_bytes, pos + batch);
		u64 n_rec = 0;
		void *out = c->pass.rec.get();
		if (c->fast) {                                   /* the batch stays resident until pass_end */
			if (fast_admit(c, kept, t0 + (u64)pos, (u64)(end - pos), (u64)(end - pos), &out)) return -1;
			if (!c->fast) { if (c->pass.rec.reserve((size_t)bmax)) return -1; out = c->pass.rec.get(); }   /* the pass has just left the fast path */
		}
		const RecFmt fmt = c->fast ? kept : consumed;
		{
			EvTimer tm(c->st);
			yk_launch_xpart((const uint8_t*)d_bases, pos, end, pos, c->k, c->pre, c->plo, c->phi, c->nb_bits,
			                c->rows, c->d_partial, c->d_bstart, out, fmt, c->st, d_valid);
			HIPCK(hipMemcpyAsync(&n_rec, c->d_bstart + ((size_t)1 << c->nb_bits), 8, hipMemcpyDeviceToHost, c->st));
			c->st_cur.ms_extract += tm.stop();
		}
		if (c->fast) { if (fast_keep(c, n_rec)) return -1; if (t0 + (u64)end > c->t_end) c->t_end = t0 + (u64)end; continue; }
		if (consume_records(c, out, fmt, (int64_t)n_rec, t0 + (u64)pos, t0 + (u64)pos, t0 + (u64)end, c->d_bstart)) return -1;
	}
	return 0;
}

extern "C" int yakamd_feed_bases_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, uint64_t t0) { return feed_image(h, d_bases, 0, n_bytes, t0); }
/* the same stream at 0.375 bytes per base: 2-bit codes, 16 bases per 32-bit word (base j at bits 2 (j % 16)), and a validity bit
 * per base (bit j % 32 of word j / 32; 0 = N, any other non-ACGT byte or a record separator).  Position j of the stream is base j */
extern "C" int yakamd_feed_packed_dev(yak_ch_t *h, const void *d_codes, const void *d_valid, int64_t n_bases, uint64_t t0)
{
	if (!d_valid) return fail("packed feed without a validity mask");
	if (((uintptr_t)d_valid & 3) != 0) return fail("validity mask must be 4-byte aligned");
	return feed_image(h, d_codes, (const u32*)d_valid, n_bases, t0);
}
extern "C" int yakamd_pack_bases_dev(const void *d_ascii, int64_t n, void *d_codes, void *d_valid, void *stream)
{
	yk_launch_pack((const uint8_t*)d_ascii, n, (u32*)d_codes, (u32*)d_valid, (hipStream_t)stream);
	return hipGetLastError() == hipSuccess ? 0 : fail("pack kernel launch failed");
}

/* the staging buffer of the host feeds: room for n bytes */
static int stage_reserve(yakamd_ctx *c, int64_t n)
{
	return (size_t)n <= c->stage.cap() ? 0 : c->stage.reserve((size_t)(n + (n >> 3) + 4096));
}

extern "C" int yakamd_feed_bases_host(yak_ch_t *h, const void *h_bases, int64_t n_bytes, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	HIPCK(hipSetDevice(c->dev));
	if (stage_reserve(c, n_bytes)) return -1;
	HIPCK(hipMemcpyAsync(c->stage, h_bases, (size_t)n_bytes, hipMemcpyHostToDevice, c->st));
	return yakamd_feed_bases_dev(h, c->stage, n_bytes, t0);
}

/* the packed image made on the host (yakamd_pack_bases_host: the code words, then -- 16-byte aligned -- the validity words): one copy of
 * 0.375 bytes per base over the bus, then the packed feed */
extern "C" int64_t yakamd_packed_bytes(int64_t n_bases) { const int64_t nw = (n_bases + 31) / 32; return ((nw * 8 + 15) & ~(int64_t)15) + nw * 4; }
extern "C" int yakamd_feed_packed_host(yak_ch_t *h, const void *h_packed, int64_t n_bases, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	if (n_bases <= 0) return 0;
	HIPCK(hipSetDevice(c->dev));
	const int64_t need = yakamd_packed_bytes(n_bases), valid_at = need - (n_bases + 31) / 32 * 4;
	if (stage_reserve(c, need)) return -1;
	HIPCK(hipMemcpyAsync(c->stage, h_packed, (size_t)need, hipMemcpyHostToDevice, c->st));
	return yakamd_feed_packed_dev(h, c->stage, c->stage + valid_at, n_bases, t0);
}

/* packed pieces of the stream, each a whole number of 32-position words (its code words and its validity words apart), laid one behind the
 * other on the device -- two copies per piece -- and fed as one image: what yak_count() does with the segments its parser threads packed */
extern "C" int yakamd_feed_packed_pieces_host(yak_ch_t *h, int n_pieces, const void *const *codes, const void *const *valid, const int64_t *n_words, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	int64_t nw = 0;
	for (int i = 0; i < n_pieces; ++i) { if (n_words[i] < 0) return fail("packed piece of negative length"); nw += n_words[i]; }
	if (nw == 0) return 0;
	HIPCK(hipSetDevice(c->dev));
	const int64_t n_bases = nw * 32, need = yakamd_packed_bytes(n_bases), valid_at = need - nw * 4;
	if (stage_reserve(c, need)) return -1;
	int64_t w = 0;
	for (int i = 0; i < n_pieces; ++i) {
		if (n_words[i] == 0) continue;
		HIPCK(hipMemcpyAsync(c->stage + w * 8, codes[i], (size_t)n_words[i] * 8, hipMemcpyHostToDevice, c->st));
		HIPCK(hipMemcpyAsync(c->stage + valid_at + w * 4, valid[i], (size_t)n_words[i] * 4, hipMemcpyHostToDevice, c->st));
		w += n_words[i];
	}
	return yakamd_feed_packed_dev(h, c->stage, c->stage + valid_at, n_bases, t0);
}

extern "C" int yakamd_feed_hashed_dev(yak_ch_t *h, const void *d_hash, const void *d_t, int64_t n, uint64_t t0, uint64_t t_span)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	HIPCK(hipSetDevice(c->dev));
	/* group the records by sub-table prefix first (same locality as the extraction path) */
	if (n <= 0) return 0;
	if (c->pass.rec.reserve((size_t)n) || part_reserve(c, yk_rpart_blocks(n))) return -1;
	u64 n_rec = 0;
	void *out = c->pass.rec.get();
	if (c->fast && fast_admit(c, YK_FMT_POS, t0, t_span, (u64)n, &out)) return -1;
	yk_launch_rpart((const u64*)d_hash, (const u32*)d_t, n, c->pre, c->plo, c->phi, c->nb_bits,
	                c->rows, c->d_partial, c->d_bstart, (Rec*)out, c->st);
	HIPCK(hipMemcpyAsync(&n_rec, c->d_bstart + ((size_t)1 << c->nb_bits), 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (c->fast) { if (t0 + t_span > c->t_end) c->t_end = t0 + t_span; return fast_keep(c, n_rec); }
	return consume_records(c, out, YK_FMT_POS, (int64_t)n_rec, t0, t0, t0 + t_span, c->d_bstart);
}

static int64_t partition_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_out, RecFmt fmt, uint64_t *h_bstart)
{
	if (k < 1 || k > 63 || pre < 3 || pre > 13) { fail("partition: unsupported k / pre"); return -1; }
	if (((uintptr_t)d_bases & 15) != 0 || n_bytes >= ((int64_t)1 << 32)) { fail("partition: base image must be 16-byte aligned and < 4 GiB"); return -1; }
	const size_t NB = (size_t)1 << pre;
	if (n_bytes <= 0) { memset(h_bstart, 0, (NB + 1) * 8); return 0; }   /* no chunk: nothing is launched (yk_launch_xpart would leave d_bstart as the pool handed it out) */
	const int n_blk = yk_xpart_blocks(n_bytes);
	DevBuf<u64> d_bstart, d_partial; DevBuf<u32> d_rows;
	if (d_rows.alloc(NB * (size_t)n_blk) || d_partial.alloc(NB * yk_part_groups()) || d_bstart.alloc(NB + 1)) return -1;
	/* on a stream of its own, not the null stream (which waits for, and holds up, every other stream of the device): a multi-GPU job partitions the
	 * chunks of its next round while the owners' streams take in the round before */
	int dev = 0;
	(void)hipGetDevice(&dev);
	hipStream_t ps = yk_stream_get(dev);
	yk_launch_xpart((const uint8_t*)d_bases, 0, n_bytes, 0, k, pre, 0, 1 << pre, pre, d_rows, d_partial, d_bstart, d_out, fmt, ps);
	hipError_t e = hipMemcpyAsync(h_bstart, d_bstart, (NB + 1) * 8, hipMemcpyDeviceToHost, ps);
	if (e == hipSuccess) e = hipStreamSynchronize(ps);
	yk_stream_put(dev, ps);
	if (e != hipSuccess) { fail("partition: %s", hipGetErrorString(e)); return -1; }
	return (int64_t)h_bstart[NB];
}

extern "C" int64_t yakamd_partition_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_rec_out, uint64_t *h_bstart)
{
	return partition_dev(k, pre, d_bases, n_bytes, d_rec_out, YK_FMT_POS, h_bstart);
}

/* the same partition as 8-byte tagged records (yk_device.h YK_R8_*: half the exchange payload of a sharded pass); for
 * yakamd_feed_partitioned_tagged_dev on the owner.  yakamd_tagged_ok says whether k / pre allow the format */
extern "C" int yakamd_tagged_ok(int k, int pre) { return k >= 1 && pre >= 3 && yk_tagged_fits(k, pre); }   /* (k and pre as partition_dev takes them) */
extern "C" int64_t yakamd_partition_tagged_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_rec8_out, uint64_t *h_bstart)
{
	if (!yakamd_tagged_ok(k, pre)) { fail("partition: tagged records need k < 32, 2k - pre <= 52, pre <= 10"); return -1; }
	if (n_bytes > ((int64_t)1 << 31)) { fail("partition: at most 2^31 stream positions per call with tagged records (31-bit run starts)"); return -1; }
	return partition_dev(k, pre, d_bases, n_bytes, d_rec8_out, YK_FMT_TAGGED, h_bstart);
}

extern "C" int64_t yakamd_partition_hashes_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_hash_out, uint64_t *h_bstart)
{
	return partition_dev(k, pre, d_bases, n_bytes, d_hash_out, YK_FMT_HASH, h_bstart);
}

static int feed_partitioned(yak_ch_t *h, const void *d_rec, RecFmt fmt, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span, bool borrow)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	if (c->nb_bits != c->pre) return fail("feed_partitioned needs pre <= 13");
	HIPCK(hipSetDevice(c->dev));
	if (n <= 0) return 0;
	const size_t NB = (size_t)1 << c->nb_bits;
	if (c->fast) {
		void *out = 0;
		if (fmt == YK_FMT_TAGGED && !(yakamd_tagged_ok(c->k, c->pre) && !c->or_mode)) return fail("tagged records do not fit this table (k, pre)");
		if (fast_admit(c, fmt, t0, t_span, (u64)n, &out, borrow ? d_rec : 0)) return -1;
		if (c->fast) {                                       /* admitted: already grouped by prefix; keep a private copy unless lent */
			if (!borrow) HIPCK(hipMemcpyAsync(out, d_rec, (size_t)n * yk_rec_bytes(fmt), hipMemcpyDeviceToDevice, c->st));
			Kept &k = c->pass.kept.back();
			k.bstart.assign(h_bstart, h_bstart + NB + 1);
			k.n = (u64)n;
			c->st_cur.n_instances += n;
			if (t0 + t_span > c->t_end) c->t_end = t0 + t_span;
			return 0;
		}
	}
	if (fmt == YK_FMT_TAGGED) return fail("tagged records need the exclusive-ownership path (the pass left it: input beyond the device budget, or YAKAMD_FAST=0)");
	return consume_records(c, d_rec, fmt, n, t0, t0, t0 + t_span);   /* general path / pass 2: consume in place */
}

extern "C" int yakamd_feed_partitioned_dev(yak_ch_t *h, const void *d_rec, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span)
{
	return feed_partitioned(h, d_rec, YK_FMT_POS, n, h_bstart, t0, t_span, false);
}

extern "C" int yakamd_feed_partitioned_lent_dev(yak_ch_t *h, const void *d_rec, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span)
{
	return feed_partitioned(h, d_rec, YK_FMT_POS, n, h_bstart, t0, t_span, true);
}

/* 1 while the open pass of h runs on the exclusive-ownership path (the only one that takes tagged records) */
extern "C" int yakamd_pass_fast(yak_ch_t *h) { yakamd_ctx *c = ctx_of(h); return c && c->in_pass && c->fast && !c->or_mode; }

extern "C" int yakamd_feed_partitioned_tagged_dev(yak_ch_t *h, const void *d_rec8, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span, int lent)
{
	return feed_partitioned(h, d_rec8, YK_FMT_TAGGED, n, h_bstart, t0, t_span, lent != 0);
}

/* ---- the hashes of a base image (the device-level exports of the lookup commands are in lookup_dev.cpp) ---- */
extern "C" int64_t yakamd_extract_dev(int k, const void *d_bases, int64_t n_bytes, void *d_hash, void *d_t,
                                      int pre, int plo, int phi, void *stream)
{
	if (k >= 64 || k < 1) { fail("extract: unsupported k"); return -1; }
	u64 *d_cur = 0, n = 0;
	hipStream_t st = (hipStream_t)stream;
	if (hipMalloc((void**)&d_cur, 8) != hipSuccess) { fail("hipMalloc"); return -1; }
	hipMemsetAsync(d_cur, 0, 8, st);
	yk_launch_extract((const uint8_t*)d_bases, 0, n_bytes, 0, k, pre, plo, phi, (u64*)d_hash, (u32*)d_t, d_cur, st);
	hipMemcpyAsync(&n, d_cur, 8, hipMemcpyDeviceToHost, st);
	hipStreamSynchronize(st);
	hipFree(d_cur);
	return (int64_t)n;
}

/* the end of a pass: pending counts folded in, or the new keys of a create pass laid out */
static int64_t pass_end_body(yakamd_ctx *c)
{
	HIPCK(hipSetDevice(c->dev));
	int64_t n_ins = 0;
	if (c->k >= 32 && yk_bad_hash_seen(c->st)) { pass_free(c); return fail("a 64-bit k-mer hash equals the empty-slot pattern: unsupported input for k >= 32"); }
	if (!c->create_new) {
		if (c->d_delta && c->delta_dirty) yk_launch_img_fold(img_view(c), c->n_slots, c->st);   /* (k_cnt2_apply writes its counts straight into the keys) */
		HIPCK(hipStreamSynchronize(c->st));
		c->d_delta.reset();
		c->host_valid = false;
		retained_drop(c);                                        /* used or not: the next pass is another input's */
	} else if (c->or_mode && !(c->fast && !c->pass.acc.s)) {
		pass_free(c);
		return fail("flag-mode loads need the exclusive-ownership path (prefix length <= 13, input within the device budget)");
	} else if (c->fast && !c->pass.acc.s) {
		if (fast_finish(c, true)) return -1;
		n_ins = (int64_t)(c->img_keys_total - c->keys_at_begin);   /* earlier slices of the pass included */
		c->st_cur.n_new_keys = n_ins;
	} else if (acc_finish(c, &n_ins)) return -1;
	pass_free(c);
	c->st_cur.ms_total = now_ms() - c->st_cur.ms_total;
	c->st_last = c->st_cur;
	return n_ins;
}

extern "C" int64_t yakamd_pass_end(yak_ch_t *h)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("no pass open");
	int64_t r = pass_end_body(c);
	if (r >= 0) {                                              /* a launch that was refused (bad configuration) reports nothing by itself */
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) r = fail("a HIP call of this pass was refused: %s", hipGetErrorString(e));
	}
	if (r < 0) pass_free(c);                                 /* a failed pass is closed too: the table stays usable (the pass's k-mers are lost, the error is reported) */
	return r;
}
