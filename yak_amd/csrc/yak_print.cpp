/*
 * yak_print.cpp -- `yak print` (reference main.c:286-323) on the device.  The stored keys of a range of sub-tables come from the table's
 * device-side .yak body (yk_ctx_dump_image_dev: ascending slot order, the order yak_ch_getseq walks) and are turned into k-mers
 * (yakamd_kmers_dev) or into the text the reference writes (yakamd_print_dev) by the kernels of kern_print.inc.  yakamd_print() lists a whole
 * table in ranges of sub-tables whose text fits a device buffer: while one range's text crosses the bus in pinned pieces and is written, the
 * next one is formatted.  No host mirror of the table is built.  A table sharded over prefix ranges is listed shard by shard in prefix order.
 */
#include "yak_host.h"
#include "yak_amd.h"

namespace {

/* a run of sub-tables [lo, hi) that one shard of a table owns */
struct Piece { yak_ch_t *s; yakamd_ctx *c; int lo, hi; };

/* [lo, hi) of `h` cut by owner, in prefix order; false after a message */
bool pieces_of(const yak_ch_t *h, int lo, int hi, const char *what, std::vector<Piece> *out)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	out->clear();
	if (!h || e->magic != EXT_MAGIC) { yk_set_error("%s: not an engine table", what); return false; }
	if (h->k < 1 || h->k >= 32) { yk_set_error("%s: k = %d: k-mers can be listed for k below 32 only (reference htab.c:359)", what, h->k); return false; }
	if (lo < 0 || hi < lo || hi > 1 << h->pre) { yk_set_error("%s: sub-tables [%d, %d) of %d", what, lo, hi, 1 << h->pre); return false; }
	const int n_sh = YK_MULTI(e) ? e->n_sub : 1;
	for (int r = 0; r < n_sh; ++r) {
		yak_ch_t *s = YK_MULTI(e) ? e->sub[r] : (yak_ch_t*)h;
		std::vector<yakamd_ctx*> eng;
		if (yk_inspect_engines(s, &eng)) return false;               /* (an engine table, out of a pass) */
		int a = 0, b = 0;
		yk_ctx_range(eng[0], &a, &b);
		a = std::max(a, lo); b = std::min(b, hi);
		if (a < b) out->push_back(Piece{ s, eng[0], a, b });
	}
	return true;
}

/* the caller's arrays are on one device: so must the shards be whose kernels write them */
bool on_one_device(const std::vector<Piece> &pcs, const char *what)
{
	for (const Piece &p : pcs)
		if (yk_ctx_device(p.c) != yk_ctx_device(pcs[0].c)) { yk_set_error("%s: the table is spread over several devices; list it shard by shard, or with yakamd_print()", what); return false; }
	return true;
}

/* one piece on its device: the .yak body of its sub-tables and the key offsets of kern_print.inc */
struct Staged {
	Piece pc;
	std::vector<u64> off;                                          /* [n_sub + 1] */
	u64 *d_img = 0, *d_off = 0, *d_toff = 0;
	u32 *d_tcnt = 0;
	u64 n = 0, bytes = 0;
	Staged() = default;
	Staged(const Staged&) = delete;
	Staged &operator=(const Staged&) = delete;
	~Staged() { drop(); }
	void drop()
	{
		if (!d_img && !d_off && !d_toff && !d_tcnt) return;
		(void)hipSetDevice(yk_ctx_device(pc.c));
		if (d_img) yk_pool_release(d_img);
		yakamd_dev_free(d_off); yakamd_dev_free(d_toff); yakamd_dev_free(d_tcnt);
		d_img = d_off = d_toff = 0; d_tcnt = 0;
	}
	void count(const Piece &p)                                     /* the sizes alone: no device work */
	{
		pc = p;
		off.assign(1, 0);
		for (int w = p.lo; w < p.hi; ++w) {
			uint32_t cap = 0, size = 0;
			yakamd_subtable(p.s, w, &cap, &size);
			off.push_back(off.back() + size);
		}
		n = off.back();
	}
	bool stage()
	{
		if (n == 0) return true;
		u64 n_words = 0;
		if (yk_ctx_dump_image_dev(pc.c, pc.lo, pc.hi, &d_img, &n_words) != 0) return false;
		if (n_words != n + (u64)(pc.hi - pc.lo)) { yk_set_error("print: the table changed while it was listed"); return false; }
		d_off = (u64*)yakamd_dev_alloc(off.size() * 8);
		if (!d_off || yakamd_memcpy_h2d(d_off, off.data(), off.size() * 8) != 0) { yk_set_error("print: no device memory for %zu offsets", off.size()); return false; }
		return true;
	}
	/* the bytes of the text: computed (without counts), or the scan of the tiles' sizes read back */
	bool measure(int k, int with_counts)
	{
		if (!with_counts || n == 0) { bytes = n * (u64)(k + 1); return true; }
		const u64 nt = yk_print_tiles(n);
		const hipStream_t st = yk_ctx_stream(pc.c);
		d_tcnt = (u32*)yakamd_dev_alloc(nt * 4);
		d_toff = (u64*)yakamd_dev_alloc((nt + 1) * 8);
		if (!d_tcnt || !d_toff) { yk_set_error("print: no device memory for %llu tile offsets", (unsigned long long)nt); return false; }
		if (yk_launch_print_sizes(d_img, d_off, n, pc.hi - pc.lo, k, d_tcnt, st) != 0) { yk_set_error("print: the size kernel did not launch"); return false; }
		yk_launch_te_scan(d_tcnt, (int64_t)nt, 1, d_toff, st);
		if (hipMemcpyAsync(&bytes, d_toff + nt, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
			yk_set_error("print: sizes: %s", hipGetErrorString(hipGetLastError()));
			return false;
		}
		return true;
	}
	bool format(int k, int pre, int with_counts, uint8_t *d_text)  /* returns when the text is there */
	{
		if (n == 0) return true;
		const hipStream_t st = yk_ctx_stream(pc.c);
		if (yk_launch_print(d_img, d_off, n, pc.hi - pc.lo, pc.lo, k, pre, with_counts, d_toff, d_text, st) != 0 || hipStreamSynchronize(st) != hipSuccess) {
			yk_set_error("print: the listing kernel failed: %s", hipGetErrorString(hipGetLastError()));
			return false;
		}
		return true;
	}
};

/* what one device lends to yakamd_print(): two text buffers, a copy stream, two pinned pieces */
struct PrintDev {
	enum { CH = 8 << 20 };
	int dev = -1;
	uint8_t *d_text[2] = { 0, 0 };
	void *pin[2] = { 0, 0 };
	hipStream_t st = 0;
	hipEvent_t ev[2] = { 0, 0 };
	bool open(int dev_, size_t text_bytes)
	{
		dev = dev_;
		if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return false;
		for (int i = 0; i < 2; ++i) {
			d_text[i] = (uint8_t*)yakamd_dev_alloc(text_bytes);
			if (!d_text[i] || hipHostMalloc(&pin[i], CH, hipHostMallocPortable) != hipSuccess || hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return false;
		}
		return true;
	}
	void close()
	{
		if (dev < 0) return;
		(void)hipSetDevice(dev);
		for (int i = 0; i < 2; ++i) { yakamd_dev_free(d_text[i]); if (pin[i]) (void)hipHostFree(pin[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); }
		if (st) (void)hipStreamDestroy(st);
		dev = -1;
	}
	/* `bytes` of d_src to fd, in order: piece j + 1 is on the bus while piece j is written */
	bool drain(const uint8_t *d_src, size_t bytes, int fd)
	{
		if (bytes == 0) return true;
		if (hipSetDevice(dev) != hipSuccess) return false;
		const size_t n_ch = (bytes + CH - 1) / CH;
		auto issue = [&](size_t j) {
			const size_t n = std::min<size_t>(CH, bytes - j * CH);
			return hipMemcpyAsync(pin[j & 1], d_src + j * CH, n, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[j & 1], st) == hipSuccess;
		};
		bool ok = issue(0);
		for (size_t j = 0; ok && j < n_ch; ++j) {
			ok = hipEventSynchronize(ev[j & 1]) == hipSuccess;
			if (ok && j + 1 < n_ch) ok = issue(j + 1);
			const size_t n = std::min<size_t>(CH, bytes - j * CH);
			for (size_t done = 0; ok && done < n; ) {
				const ssize_t r = ::write(fd, (const char*)pin[j & 1] + done, n - done);
				if (r <= 0) ok = false; else done += (size_t)r;
			}
		}
		(void)hipStreamSynchronize(st);
		return ok;
	}
};

}   // namespace

extern "C" int64_t yakamd_kmers_dev(yak_ch_t *h, int sub_lo, int sub_hi, void *d_x_u64, void *d_c_u16, int64_t cap)
{
	std::vector<Piece> pcs;
	if (!pieces_of(h, sub_lo, sub_hi, "kmers", &pcs) || !on_one_device(pcs, "kmers")) return -1;
	std::vector<Staged> st(pcs.size());
	u64 n = 0;
	for (size_t i = 0; i < pcs.size(); ++i) { st[i].count(pcs[i]); n += st[i].n; }
	if (!d_x_u64 || !d_c_u16 || cap < (int64_t)n) return (int64_t)n;
	if (((uintptr_t)d_x_u64 & 7) != 0 || ((uintptr_t)d_c_u16 & 1) != 0) return yk_set_error("kmers: the output arrays must be 8- and 2-byte aligned");
	u64 at = 0;
	for (Staged &s : st) {
		if (s.n == 0) continue;
		if (!s.stage()) return -1;
		const hipStream_t q = yk_ctx_stream(s.pc.c);
		if (yk_launch_kmers(s.d_img, s.d_off, s.n, s.pc.hi - s.pc.lo, s.pc.lo, h->k, h->pre, (u64*)d_x_u64 + at, (unsigned short*)d_c_u16 + at, q) != 0
		    || hipStreamSynchronize(q) != hipSuccess) return yk_set_error("kmers: the listing kernel failed: %s", hipGetErrorString(hipGetLastError()));
		at += s.n;
		s.drop();
	}
	return (int64_t)n;
}

extern "C" int64_t yakamd_print_dev(yak_ch_t *h, int sub_lo, int sub_hi, int with_counts, void *d_text, int64_t cap_bytes)
{
	std::vector<Piece> pcs;
	if (!pieces_of(h, sub_lo, sub_hi, "print", &pcs) || !on_one_device(pcs, "print")) return -1;
	std::vector<Staged> st(pcs.size());
	u64 bytes = 0;
	for (size_t i = 0; i < pcs.size(); ++i) {
		st[i].count(pcs[i]);
		if (with_counts && !st[i].stage()) return -1;               /* with counts the line lengths are the device's to tell */
		if (!st[i].measure(h->k, with_counts)) return -1;
		bytes += st[i].bytes;
	}
	if (!d_text || cap_bytes < (int64_t)bytes) return (int64_t)bytes;
	u64 at = 0;
	for (Staged &s : st) {
		if (s.n == 0) continue;
		if (!with_counts && !s.stage()) return -1;
		if (!s.format(h->k, h->pre, with_counts, (uint8_t*)d_text + at)) return -1;
		at += s.bytes;
		s.drop();
	}
	return (int64_t)bytes;
}

extern "C" void yakamd_propt_init(yakamd_propt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_propt_t));
	opt->with_counts = 0;
	opt->n_threads = 4;
	opt->batch_bytes = (int64_t)256 << 20;
}

extern "C" int yakamd_print(const yakamd_propt_t *opt, const yak_ch_t *ch, const char *out_fn)
{
	std::vector<Piece> pcs;
	if (!pieces_of(ch, 0, ch ? 1 << ch->pre : 0, "print", &pcs)) return -1;
	const int k = ch->k, pre = ch->pre, with_counts = opt->with_counts != 0;
	const u64 line_max = (u64)k + (with_counts ? 6 : 1);
	const u64 room = (u64)std::max<int64_t>(opt->batch_bytes, 1) / line_max;   /* keys per range */
	/* the ranges: as many whole sub-tables of one shard as `room` keys allow, one at the least */
	std::vector<Piece> ranges;
	u64 most = 0;
	for (const Piece &p : pcs) {
		int lo = p.lo;
		u64 n = 0;
		for (int w = p.lo; w < p.hi; ++w) {
			uint32_t cap = 0, size = 0;
			yakamd_subtable(p.s, w, &cap, &size);
			if (w > lo && n + size > room) { ranges.push_back(Piece{ p.s, p.c, lo, w }); most = std::max(most, n); lo = w; n = 0; }
			n += size;
		}
		ranges.push_back(Piece{ p.s, p.c, lo, p.hi });
		most = std::max(most, n);
	}
	const bool to_stdout = !out_fn || strcmp(out_fn, "-") == 0;
	if (to_stdout) fflush(stdout);
	const int fd = to_stdout ? STDOUT_FILENO : ::open(out_fn, O_WRONLY | O_CREAT | O_TRUNC, 0666);
	if (fd < 0) return yk_set_error("print: cannot write '%s'", out_fn);
	const double t0 = yk_realtime();
	std::map<int, PrintDev> devs;
	std::thread writer;
	bool ok = true, wrote = true;
	u64 total = 0;
	double t_fmt = 0;
	int turn = 0;                                                  /* ranges that had text: they alternate between the two buffers */
	for (size_t r = 0; ok && r < ranges.size(); ++r) {
		Staged s;
		s.count(ranges[r]);
		if (s.n == 0) continue;
		const int dev = yk_ctx_device(s.pc.c);
		if (!devs.count(dev) && !devs[dev].open(dev, (size_t)(most * line_max + 16))) { ok = false; yk_set_error("print: no device memory for two text buffers of %llu bytes", (unsigned long long)(most * line_max)); break; }
		PrintDev &pd = devs[dev];
		const double a = yk_realtime();
		/* this buffer was drained by the writer before the last one, joined before the last range was handed over */
		uint8_t *d_text = pd.d_text[turn++ & 1];
		ok = s.stage() && s.measure(k, with_counts) && s.bytes <= most * line_max && s.format(k, pre, with_counts, d_text);
		t_fmt += yk_realtime() - a;
		if (writer.joinable()) writer.join();
		ok = ok && wrote;
		if (!ok) break;
		const size_t nb = (size_t)s.bytes;
		total += nb;
		PrintDev *pdp = &pd;
		writer = std::thread([pdp, d_text, nb, fd, &wrote]() { wrote = pdp->drain(d_text, nb, fd); });
	}
	if (writer.joinable()) writer.join();
	if (ok && !wrote) { ok = false; yk_set_error("print: the copy or the write of the text failed"); }
	for (auto &kv : devs) kv.second.close();
	if (!to_stdout && ::close(fd) != 0 && ok) { ok = false; yk_set_error("print: cannot write '%s'", out_fn); }
	if (ok && getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] print: %.1f MB of text in %zu ranges, %.3f s (%.3f s of it staging and formatting)\n", total / 1e6, ranges.size(), yk_realtime() - t0, t_fmt);
	return ok ? 0 : -1;
}
