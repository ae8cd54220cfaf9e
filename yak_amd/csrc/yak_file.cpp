/*
 * yak_file.cpp -- tables to and from the .yak format (include/yak.h: yak_ch_dump, yak_ch_restore, yak_ch_restore_core; include/yak_amd.h:
 * yakamd_dump_mem, yakamd_dump_range_mem, yakamd_yak_header).  The dump puts the bytes together on the device and writes them; the restore reads
 * a file through yak_file.h, the format's one reader, and words its messages here.
 */
#include "yak_host.h"
#include "yak_file.h"

/* ---- .yak serialisation (reference htab.c:373-394): header, then per sub-table capacity, size and
 * the keys in ascending slot order.  Every shard puts the bytes of its own sub-tables together on its device
 * (StagedRange); they come back in one copy (yakamd_dump_mem), or go to the file in 8 MiB pieces through a
 * few page-locked buffers that writer threads pwrite() while the next pieces are on the bus (yak_ch_dump) ---- */
struct DumpSink {
	uint8_t *mem; int fd;                                      /* one of the two */
	bool put(int dev, hipStream_t st, const uint8_t *d_src, size_t bytes, size_t off);
};
bool DumpSink::put(int dev, hipStream_t st, const uint8_t *d_src, size_t bytes, size_t off)
{
	if (bytes == 0) return true;
	if (hipSetDevice(dev) != hipSuccess) return false;            /* the events below are recorded on `st`: they must be this device's */
	if (mem) return hipMemcpyAsync(mem + off, d_src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
	enum { NB = 6, W = 3 };
	const size_t CH = (size_t)8 << 20, n_ch = (bytes + CH - 1) / CH;
	static std::mutex mu;                                         /* the staging buffers are the process's: one dump at a time uses them */
	static void *stage[NB] = { 0 };
	std::lock_guard<std::mutex> lk(mu);
	for (int i = 0; i < NB; ++i) if (!stage[i] && hipHostMalloc(&stage[i], CH, hipHostMallocPortable) != hipSuccess) { stage[i] = 0; return false; }
	hipEvent_t ev[NB];
	for (int i = 0; i < NB; ++i) if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) { while (i-- > 0) (void)hipEventDestroy(ev[i]); return false; }
	std::vector<int> issued_v(n_ch, 0), written_v(n_ch, 0);
	volatile int *issued = issued_v.data(), *written = written_v.data();
	bool good = true;
	std::vector<std::thread> th;
	for (int w = 0; w < W; ++w) th.emplace_back([&, w]() {
		(void)hipSetDevice(dev);
		for (size_t j = (size_t)w; j < n_ch; j += W) {
			while (!__atomic_load_n(&issued[j], __ATOMIC_ACQUIRE)) std::this_thread::yield();
			bool ok = __atomic_load_n(&issued[j], __ATOMIC_ACQUIRE) == 1 && hipEventSynchronize(ev[j % NB]) == hipSuccess;
			const size_t n = std::min(CH, bytes - j * CH);
			for (size_t done = 0; ok && done < n; ) {
				const ssize_t r = ::pwrite(fd, (const char*)stage[j % NB] + done, n - done, (off_t)(off + j * CH + done));
				if (r <= 0) ok = false; else done += (size_t)r;
			}
			if (!ok) __atomic_store_n(&good, false, __ATOMIC_RELAXED);
			__atomic_store_n(&written[j], 1, __ATOMIC_RELEASE);
		}
	});
	for (size_t i = 0; i < n_ch; ++i) {
		if (i >= NB) while (!__atomic_load_n(&written[i - NB], __ATOMIC_ACQUIRE)) std::this_thread::yield();
		const size_t n = std::min(CH, bytes - i * CH);
		const bool ok = hipMemcpyAsync(stage[i % NB], d_src + i * CH, n, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[i % NB], st) == hipSuccess;
		__atomic_store_n(&issued[i], ok ? 1 : 2, __ATOMIC_RELEASE);
	}
	for (auto &t : th) t.join();
	(void)hipStreamSynchronize(st);
	for (int i = 0; i < NB; ++i) (void)hipEventDestroy(ev[i]);
	return good;
}

/* the bytes of sub-tables [lo, hi) -- {capacity, size, keys in slot order} each -- through `sink`, behind the 16-byte header when `head` is set (the whole
 * table then: the .yak image), every shard staging the part it owns; their number, or -1.  sink == 0: the number alone */
static int64_t dump_through(yak_ch_t *h, int lo, int hi, bool head, DumpSink *sink)
{
	yak_ch_ext *e = (yak_ch_ext*)h;
	const int P = 1 << h->pre, n_sub = YK_MULTI(e) ? e->n_sub : 1;
	if (lo < 0 || hi > P || lo >= hi) return -1;
	struct Part { yak_ch_t *hs; int a, b; };
	std::vector<Part> part;
	size_t sz = (head ? 16 : 0) + (size_t)8 * (hi - lo), off = 0;
	uint32_t cap, cnt;
	for (int r = 0; r < n_sub; ++r) {
		const ShardSpan own = yk_shard_span(h->pre, n_sub, r);
		const Part pt = { YK_MULTI(e) ? e->sub[r] : h, std::max(lo, own.lo), std::min(hi, own.hi) };
		for (int p = pt.a; p < pt.b; ++p) { if (yakamd_subtable(pt.hs, p, &cap, &cnt) != 0) return -1; sz += (size_t)8 * cnt; }
		if (pt.a < pt.b) part.push_back(pt);
	}
	if (!sink) return (int64_t)sz;
	if (head) {
		uint8_t hd[16];
		const uint32_t t[3] = { (uint32_t)h->k, (uint32_t)h->pre, YAK_COUNTER_BITS };
		memcpy(hd, YAK_MAGIC, 4); memcpy(hd + 4, t, 12);
		if (sink->mem) memcpy(sink->mem, hd, 16);
		else if (::pwrite(sink->fd, hd, 16, 0) != 16) return -1;
		off = 16;
	}
	for (const Part &pt : part) {
		yakamd_ctx *c = ((yak_ch_ext*)pt.hs)->ctx;
		StagedRange s;                                               /* (the image goes back when the shard is written) */
		if (s.stage(c, pt.a, pt.b) != 0 || off + (size_t)s.n_words * 8 > sz || !sink->put(yk_ctx_device(c), yk_ctx_stream(c), (const uint8_t*)s.d_img, (size_t)s.n_words * 8, off)) return -1;
		off += (size_t)s.n_words * 8;
	}
	return off == sz ? (int64_t)sz : -1;
}

/* to memory: the whole image (yakamd_dump_mem), or the bytes of sub-tables [lo, hi) alone, no header: what one rank of a prefix-sharded job owns of
 * the .yak file (tests and bench.py compare a rank's share with the oracle's without serialising the whole table) */
static int64_t dump_to_mem(yak_ch_t *h, int lo, int hi, bool head, uint8_t **out)
{
	*out = 0;
	const int64_t sz = dump_through(h, lo, hi, head, 0);
	if (sz < 0) return -1;
	DumpSink sink; sink.mem = (uint8_t*)malloc((size_t)sz); sink.fd = -1;
	if (!sink.mem) return -1;
	if (dump_through(h, lo, hi, head, &sink) != sz) { free(sink.mem); return -1; }
	*out = sink.mem;
	return sz;
}

/* a .yak file for restore (htab.c:413-433): the header within restore's limits -- it allocates 1 << pre descriptors, so pre is at most 24 --, then
 * per sub-table capacity, size and keys.  false after restore's message, where it has one */
static bool read_table_file(const char *fn, YakHeader *hd, std::vector<uint32_t> &caps, std::vector<uint32_t> &sizes, std::vector<uint64_t> &keys)
{
	FILE *fp = fopen(fn, "rb");
	if (fp == 0) return false;
	YakSrc src = YakSrc::file(fp);
	YakBody at;
	bool ok = false;
	const YakStatus st = yak_read_header(src, hd);
	if (st == YAK_BAD_MAGIC) fprintf(stderr, "ERROR: wrong file magic.\n");
	else if (st == YAK_BAD_BITS) fprintf(stderr, "ERROR: saved counter bits: %d; compile-time counter bits: %d\n", hd->bits, YAK_COUNTER_BITS);
	else if (st == YAK_OK && hd->pre >= YAK_COUNTER_BITS && hd->pre <= 24) {   /* (a short header or another pre: refused without a message, as they were) */
		const YakStatus body = yak_read_all(src, (int)hd->pre, caps, sizes, keys, &at);
		if (body == YAK_BAD_SUBTABLE) fprintf(stderr, "ERROR: corrupt sub-table header in '%s' (capacity %u, size %u)\n", fn, at.cap, at.size);
		else if (body == YAK_TRUNCATED) fprintf(stderr, "ERROR: '%s' is truncated at sub-table %d\n", fn, at.cur);
		ok = body == YAK_OK;
	}
	fclose(fp);
	return ok;
}

extern "C" {

int64_t yakamd_dump_mem(yak_ch_t *h, uint8_t **out) { return dump_to_mem(h, 0, 1 << h->pre, true, out); }
int64_t yakamd_dump_range_mem(yak_ch_t *h, int lo, int hi, uint8_t **out) { return dump_to_mem(h, lo, hi, false, out); }

int yak_ch_dump(const yak_ch_t *h, const char *fn)
{
	struct stat sb;
	const bool to_stdout = strcmp(fn, "-") == 0;
	if (to_stdout || (stat(fn, &sb) == 0 && !S_ISREG(sb.st_mode))) {   /* a pipe (or any name that is no regular file) takes the image in one piece */
		FILE *fp = to_stdout ? stdout : fopen(fn, "wb");
		if (fp == 0) return -1;
		uint8_t *buf = 0;
		const int64_t sz = yakamd_dump_mem((yak_ch_t*)h, &buf);
		if (sz < 0) { if (!to_stdout) fclose(fp); return -1; }
		const bool ok = fwrite(buf, 1, (size_t)sz, fp) == (size_t)sz;
		free(buf);
		if ((to_stdout ? fflush(fp) : fclose(fp)) != 0 || !ok) return -1;
	} else {
		const double t0 = yk_realtime();
		DumpSink sink; sink.mem = 0;
		/* fopen(fn, "wb"), htab.c:377 -- except that a file that is there is cut to the new size AFTER it was written over: its pages are reused
		 * instead of being given back and asked for again (0.05 s instead of 0.12 s for 420 MB) */
		sink.fd = ::open(fn, O_WRONLY | O_CREAT, 0666);
		if (sink.fd < 0) return -1;
		const int64_t sz = dump_through((yak_ch_t*)h, 0, 1 << h->pre, true, &sink);
		const bool cut = sz >= 0 && ::ftruncate(sink.fd, (off_t)sz) == 0;
		if (sz < 0) (void)::ftruncate(sink.fd, 0);                  /* a dump that failed midway leaves an empty file, not a header in front of old bytes (fopen "wb", htab.c:377, never keeps any) */
		if (::close(sink.fd) != 0 || !cut) return -1;
		if (getenv("YAKAMD_VERBOSE")) fprintf(stderr, "[yak_amd] dump: %.1f MB in %.3f s\n", sz / 1e6, yk_realtime() - t0);
	}
	fprintf(stderr, "[M::%s] dumpped the hash table to file '%s'.\n", __func__, fn);
	return 0;
}

/* include/yak_amd.h: k and pre of a .yak file's header, for a command that checks its tables against each other before it loads any.  The counter
 * bits are left to the load, which words their refusal.  No device call */
int yakamd_yak_header(const char *fn, int *k, int *pre)
{
	FILE *fp = fopen(fn, "rb");
	if (!fp) return yk_set_error("yak header: cannot open '%s'", fn);
	YakSrc src = YakSrc::file(fp);
	YakHeader hd;
	const YakStatus st = yak_read_header(src, &hd);
	fclose(fp);
	if (st == YAK_SHORT_HEADER) return yk_set_error("yak header: '%s': truncated header", fn);
	if (st == YAK_BAD_MAGIC) return yk_set_error("yak header: '%s': wrong file magic", fn);
	*k = (int)hd.k; *pre = (int)hd.pre;
	return 0;
}

/* reference htab.c:396-476.  YAK_LOAD_ALL builds the table from the file: every sub-table is pre-sized to the saved
 * capacity and the keys are put back in file order -- the same staged FCFS replay as shrink; the flag modes (trio binning
 * 2 / 3 with min_cnt, mid_cnt; sex chromosomes 4 / 5 / 6) put every selected key with a flag in its low
 * bits, ORing the flag into keys already present -- one counting pass on the device whose records
 * carry the flag in the low 4 bits of their list position.  The file is read, and refused, before any device call. */
yak_ch_t *yak_ch_restore_core(yak_ch_t *ch0, const char *fn, int mode, ...)
{
	int min_cnt = 0, mid_cnt = 0;
	va_list ap;
	va_start(ap, mode);
	if (mode == YAK_LOAD_TRIOBIN1 || mode == YAK_LOAD_TRIOBIN2) { min_cnt = va_arg(ap, int); mid_cnt = va_arg(ap, int); }
	va_end(ap);
	if (mode < YAK_LOAD_ALL || mode > YAK_LOAD_SEXCHR3) return 0;
	if (ch0 == 0 && (mode == YAK_LOAD_TRIOBIN2 || mode == YAK_LOAD_SEXCHR2 || mode == YAK_LOAD_SEXCHR3)) return 0;   /* htab.c:413-420 */
	YakHeader hd;
	std::vector<uint32_t> caps, sizes;
	std::vector<uint64_t> keys;
	if (!read_table_file(fn, &hd, caps, sizes, keys)) return 0;
	if (mode == YAK_LOAD_ALL && ch0 == 0) {
		yak_ch_t *h = yak_ch_init((int)hd.k, (int)hd.pre, 0, 0);
		if (h == 0) return 0;
		if (yk_ctx_load(((yak_ch_ext*)h)->ctx, caps.data(), sizes.data(), keys.data()) != 0) { yak_ch_destroy(h); return 0; }
		fprintf(stderr, "[M::%s] inserted %ld k-mers, of which %ld are new\n", __func__, (long)keys.size(), (long)keys.size());
		return h;
	}
	/* every other case puts the selected keys, in file order, into a table that may already hold some of them
	 * (htab.c:441-470): a flag mode ORs a flag into keys already present, YAK_LOAD_ALL leaves them alone, and a
	 * new key keeps the flag / its saved count.  That is a counting pass whose records carry the payload in the low
	 * bits of their list position (4 bits for a flag, 10 for a count), run in as many passes as the 32-bit
	 * position field needs: a pass meets the keys of the earlier ones as existing state, exactly as the
	 * reference's sequential puts do. */
	if (ch0 && multi_refuse(ch0, __func__)) return 0;           /* a load into a table sharded over prefix ranges: not carried out shard by shard (yet) */
	yak_ch_t *h = ch0 ? ch0 : yak_ch_init((int)hd.k, (int)hd.pre, 0, 0);
	if (h == 0) return 0;
	assert((int)hd.k == h->k && (int)hd.pre == h->pre);         /* htab.c:437 */
	yakamd_ctx *c = ((yak_ch_ext*)h)->ctx;
	const int P = 1 << h->pre;
	const uint64_t mask = (1ULL << YAK_COUNTER_BITS) - 1;
	const int pbits = mode == YAK_LOAD_ALL ? YAK_COUNTER_BITS : 4;
	size_t per_pass = ((size_t)1 << (32 - pbits)) - 16;
	if (yk_knob("YAKAMD_LOAD_SLICE", 0) > 0) per_pass = std::min<size_t>(per_pass, (size_t)yk_knob("YAKAMD_LOAD_SLICE", 0));   /* tests */
	std::vector<uint64_t> hashes;
	std::vector<uint32_t> times;
	long n_tot = 0, n_new = 0;
	bool ok = yk_ctx_resize_to(c, caps.data()) == 0;             /* htab.c:441 */
	void *d_h = 0, *d_t = 0;
	auto flush = [&]() {
		const size_t n = hashes.size();
		if (n == 0 || !ok) return;
		if (!d_h) { d_h = yakamd_dev_alloc(std::min(per_pass, keys.size()) * 8); d_t = yakamd_dev_alloc(std::min(per_pass, keys.size()) * 4); }
		ok = d_h && d_t && yakamd_memcpy_h2d(d_h, hashes.data(), n * 8) == 0 && yakamd_memcpy_h2d(d_t, times.data(), n * 4) == 0;
		if (ok) {
			yk_ctx_gate(c, false); yk_ctx_or_mode(c, mode == YAK_LOAD_ALL ? 2 : 1);
			ok = yakamd_pass_begin(h, 1) == 0;
			if (ok) {
				ok = yakamd_feed_hashed_dev(h, d_h, d_t, (int64_t)n, 0, (uint64_t)n << pbits) == 0;
				const int64_t r = yakamd_pass_end(h);
				ok = ok && r >= 0;
				if (ok) n_new += (long)r;
			}
			yk_ctx_gate(c, true); yk_ctx_or_mode(c, 0);
		}
		n_tot += (long)n;
		hashes.clear(); times.clear();
	};
	size_t at = 0;
	for (int p = 0; p < P && ok; ++p)
		for (uint32_t j = 0; j < sizes[p] && ok; ++j, ++at) {
			const uint64_t key = keys[at];
			int x;
			if (mode == YAK_LOAD_ALL) x = (int)(key & mask);
			else if (mode == YAK_LOAD_TRIOBIN1 || mode == YAK_LOAD_TRIOBIN2) {
				const int cnt = (int)(key & mask), shift = mode == YAK_LOAD_TRIOBIN1 ? 0 : 2;
				x = cnt >= mid_cnt ? 2 << shift : cnt >= min_cnt ? 1 << shift : -1;
			} else x = 1 << (mode - YAK_LOAD_SEXCHR1);
			if (x < 0) continue;
			hashes.push_back((key >> YAK_COUNTER_BITS) << h->pre | (uint64_t)p);
			times.push_back((uint32_t)(hashes.size() - 1) << pbits | (uint32_t)x);
			if (hashes.size() >= per_pass) flush();
		}
	flush();
	yakamd_dev_free(d_h); yakamd_dev_free(d_t);
	if (!ok) { fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error()); if (!ch0) yak_ch_destroy(h); return 0; }
	fprintf(stderr, "[M::%s] inserted %ld k-mers, of which %ld are new\n", __func__, n_tot, n_new);
	return h;
}

yak_ch_t *yak_ch_restore(const char *fn) { return yak_ch_restore_core(0, fn, YAK_LOAD_ALL); }   /* reference htab.c:478 */

} /* extern "C" */
