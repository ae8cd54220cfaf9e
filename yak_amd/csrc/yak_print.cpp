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

typedef TablePiece Piece;

/* [lo, hi) of `h` cut by owner (yk_table_pieces), after print's own refusal: a stored key inverts to its k-mer for k below 32 only */
bool pieces_of(const yak_ch_t *h, int lo, int hi, const char *what, std::vector<Piece> *out)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	if (h && e->magic == EXT_MAGIC && (h->k < 1 || h->k >= 32)) { yk_set_error("%s: k = %d: k-mers can be listed for k below 32 only (reference htab.c:359)", what, h->k); return false; }
	return yk_table_pieces(h, lo, hi, what, out);
}

/* the caller's arrays are on one device: so must the shards be whose kernels write them */
bool on_one_device(const std::vector<Piece> &pcs, const char *what)
{
	for (const Piece &p : pcs)
		if (yk_ctx_device(p.c) != yk_ctx_device(pcs[0].c)) { yk_set_error("%s: the table is spread over several devices; list it shard by shard, or with yakamd_print()", what); return false; }
	return true;
}

/* one range of sub-tables of one shard: its sizes, its staged keys with the key offsets of kern_print.inc, and the scratch of the text's tile
 * sizes.  The device buffers are kept from one range to the next (of one device: PrintDev) */
struct Staged {
	yakamd_ctx *c = 0;
	TableRange r;
	StagedRange img;
	GrowBuf tcnt, toff;                                            /* with counts: the tiles' bytes and their scan */
	u64 n = 0, bytes = 0;
	void count(yakamd_ctx *c_, const TableRange &r_) { c = c_; r = r_; n = r.n(); }   /* the sizes alone: no device work */
	void count(const Piece &p) { count(p.c, yk_ctx_ranges(p.c, p.lo, p.hi, INT64_MAX, true)[0]); }   /* a whole piece as one range */
	bool stage() { return n == 0 || img.stage(c, r.lo, r.hi, &r.off, "print", "listed") == 0; }
	void drop() { img.drop(); }
	/* the bytes of the text: computed (without counts), or the scan of the tiles' sizes read back */
	bool measure(int k, int with_counts)
	{
		if (!with_counts || n == 0) { bytes = n * (u64)(k + 1); return true; }
		const u64 nt = yk_print_tiles(n);
		const hipStream_t st = yk_ctx_stream(c);
		if (!tcnt.fit(nt * 4) || !toff.fit((nt + 1) * 8)) { yk_set_error("print: no device memory for %llu tile offsets", (unsigned long long)nt); return false; }
		if (yk_launch_print_sizes(img.d_img, img.off(), n, r.hi - r.lo, k, (u32*)tcnt.p, st) != 0) { yk_set_error("print: the size kernel did not launch"); return false; }
		yk_launch_te_scan((const u32*)tcnt.p, (int64_t)nt, 1, (u64*)toff.p, st);
		if (hipMemcpyAsync(&bytes, (const u64*)toff.p + nt, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
			yk_set_error("print: sizes: %s", hipGetErrorString(hipGetLastError()));
			return false;
		}
		return true;
	}
	bool format(int k, int pre, int with_counts, uint8_t *d_text)  /* returns when the text is there */
	{
		if (n == 0) return true;
		const hipStream_t st = yk_ctx_stream(c);
		if (yk_launch_print(img.d_img, img.off(), n, r.hi - r.lo, r.lo, k, pre, with_counts, with_counts ? (const u64*)toff.p : 0, d_text, st) != 0 || hipStreamSynchronize(st) != hipSuccess) {
			yk_set_error("print: the listing kernel failed: %s", hipGetErrorString(hipGetLastError()));
			return false;
		}
		return true;
	}
};

/* what one device lends to yakamd_print(): the staging of its ranges, two text buffers, a copy stream, two pinned pieces */
struct PrintDev {
	enum { CH = 8 << 20 };
	int dev = -1;
	Staged s;
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
		const hipStream_t q = yk_ctx_stream(s.c);
		if (yk_launch_kmers(s.img.d_img, s.img.off(), s.n, s.r.hi - s.r.lo, s.r.lo, h->k, h->pre, (u64*)d_x_u64 + at, (unsigned short*)d_c_u16 + at, q) != 0
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
	/* the ranges: as many whole sub-tables of one shard as `room` keys allow, one at the least (table_ranges.h) */
	struct ShardRange { yakamd_ctx *c; TableRange r; };
	std::vector<ShardRange> ranges;
	u64 most = 0;
	for (const Piece &p : pcs)
		for (const TableRange &r : yk_ctx_ranges(p.c, p.lo, p.hi, (int64_t)room, true)) { ranges.push_back(ShardRange{ p.c, r }); most = std::max(most, r.n()); }
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
		if (ranges[r].r.n() == 0) continue;
		const int dev = yk_ctx_device(ranges[r].c);
		if (!devs.count(dev) && !devs[dev].open(dev, (size_t)(most * line_max + 16))) { ok = false; yk_set_error("print: no device memory for two text buffers of %llu bytes", (unsigned long long)(most * line_max)); break; }
		PrintDev &pd = devs[dev];
		Staged &s = pd.s;
		s.count(ranges[r].c, ranges[r].r);
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
