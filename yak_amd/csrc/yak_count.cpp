/*
 * yak_count.cpp -- yak_count() on one device (reference count.c:88-166), its homopolymer-compressed form and yak_recount(): the file's pieces come
 * from the input front end (SeqInput, yak_host.h) and go to the engine's feeds; a job for several ranks is handed to yak_multi.cpp.
 */
#include "yak_host.h"

extern "C" {

/* hpc: a new table is marked as living in homopolymer-compressed space before its first feed (yakamd_count_hpc); an existing table's own mark governs */
static yak_ch_t *count_file(const char *fn, const yak_copt_t *opt, yak_ch_t *h0, bool hpc)
{
	{
		std::vector<int> dev;
		const int N = h0 ? ((yak_ch_ext*)h0)->n_sub : multi_gpus(opt, &dev, fn);
		if (N > 1) {
			if (h0) { dev.clear(); for (int r = 0; r < N; ++r) dev.push_back(yk_ctx_device(((yak_ch_ext*)((yak_ch_ext*)h0)->sub[r])->ctx)); }
			return yak_count_multi(fn, opt, h0, N, dev, hpc);
		}
	}
	/* the file's identity: the filtered protocol counts the same file twice (main.c:53-57); the first call then keeps its hashed k-mers on
	 * the device (yakamd_retain_input) and the second counts those instead of parsing, copying and hashing the file again */
	uint64_t sid[4] = { 0, 0, 0, 0 };
	bool have_sid = false;
	{
		struct stat sb;
		if (fn && strcmp(fn, "-") != 0 && stat(fn, &sb) == 0 && S_ISREG(sb.st_mode) && !yk_knob("YAKAMD_NO_RETAIN", 0)) {
			sid[0] = (uint64_t)sb.st_dev; sid[1] = (uint64_t)sb.st_ino; sid[2] = (uint64_t)sb.st_size;
			sid[3] = (uint64_t)sb.st_mtim.tv_sec * 1000000000ull + (uint64_t)sb.st_mtim.tv_nsec;
			have_sid = true;
		}
	}
	bool pass_open = false;
	if (h0) {
		assert(h0->k == opt->k && h0->pre == opt->pre);         /* count.c:157 */
		int64_t n_seq_kept = 0;
		if (have_sid && yk_ctx_same_source(((yak_ch_ext*)h0)->ctx, sid, &n_seq_kept)) {
			yk_realtime();
			if (yakamd_pass_begin(h0, 0) != 0) return 0;
			const int r = yakamd_count_retained(h0);
			if (r < 0) { yakamd_pass_end(h0); return 0; }
			if (r == 0) {
				const int64_t n_ins = yakamd_pass_end(h0);
				if (n_ins < 0) return 0;
				h0->tot += (uint64_t)n_ins;
				fprintf(stderr, "[M::%s::%.3f*%.2f] %ld sequences in total (the k-mers of the first pass over this file, kept on the device); %ld distinct k-mers in the hash table\n", "yak_count",
				        yk_realtime(), yk_cputime() / (yk_realtime() + 1e-9), (long)n_seq_kept, (long)h0->tot);
				return h0;
			}
			pass_open = true;                                     /* nothing usable was kept: the pass goes on with the file */
		}
	}
	/* a plain or block-gzipped regular file is parsed by several threads, an ordinary gzip file inflated by them; anything else (a pipe) streams through the reader */
	SeqInput in;
	if (!in.open(fn, parse_threads(opt->n_thread), 1 << 20)) { if (pass_open) yakamd_pass_end(h0); return 0; }   /* count.c:152 */
	const bool parallel = in.kind != SeqInput::STREAM;
	yak_ch_t *h = h0;
	const int create_new = h0 ? 0 : 1;
	yk_realtime();
	int ok = 0;
	auto open_table = [&]() {                                /* a new table: runtime start-up, the filter's 2^bf_shift bits, the pass */
		if (!h0) h = yak_ch_init(opt->k, opt->pre, opt->bf_n_hash, opt->bf_shift);
		if (!h0 && h && hpc) yakamd_ch_set_hpc(h, 1);
		if (!h0 && h && have_sid && opt->bf_shift > opt->pre) yakamd_retain_input(h, 1);   /* a filtered count: a second pass over this file is to be expected */
		ok = h != 0 && (pass_open || yakamd_pass_begin(h, create_new) == 0);
	};
	std::thread opener;                                      /* ... happen while the first window of the file is being parsed */
	if (parallel && !h0) opener = std::thread(open_table); else open_table();
	if (!opener.joinable() && h == 0) return 0;
	uint64_t t0 = 0;
	int64_t n_seq_tot = 0;
	const bool pack = parallel && !yk_knob("YAKAMD_NO_HOST_PACK", 0);   /* the stream crosses the bus at 0.375 B per base, packed by the threads that parsed it */
	double t_sink = 0, t_open_wait = 0;
	const ImgSink sink = [&](const char *img, size_t img_n, int64_t ns, const WinPack *packed) {   /* a window's pieces, or a chunk of the streaming reader */
		const double ts0 = yk_realtime();
		if (opener.joinable()) { opener.join(); t_open_wait = yk_realtime() - ts0; }
		if (!ok) return false;
		bool good = img_n == 0 || (pack ? yakamd_feed_packed_pieces_host(h, (int)packed->n_words.size(), packed->codes.data(), packed->valid.data(), packed->n_words.data(), t0)
		                                : yakamd_feed_bases_host(h, img, (int64_t)img_n, t0)) == 0;
		t_sink += yk_realtime() - ts0;
		t0 += img_n; n_seq_tot += ns;
		fprintf(stderr, "[M::%s::%.3f*%.2f] processed %ld sequences\n", "yak_count", yk_realtime(), yk_cputime() / (yk_realtime() + 1e-9), (long)ns);
		return good;
	};
	if (parallel) {
		g_t_parse_windows.store(0, std::memory_order_relaxed);
		const double tp0 = yk_realtime();
		const bool parsed = in.run(opt->k, pack, sink);
		if (getenv("YAKAMD_VERBOSE")) fprintf(stderr, "[yak_amd] reader: %.3f s from the first window to the last piece fed; the windows took %.3f s to parse (the first %.3f s), the feeds %.3f s (%.3f s of it waiting for the new table)\n",
		                                      yk_realtime() - tp0, g_t_parse_windows.load(), g_t_first_window.load(), t_sink, t_open_wait);
		if (opener.joinable()) opener.join();
		if (h == 0) return 0;
		ok = ok && parsed;
	} else if (ok) {
		/* count.c:106: a chunk closes at chunk_size bases (and before its image outgrows a feed) */
		const PieceEnd end = { opt->chunk_size, (size_t)1 << 31 };
		ok = in.stream(opt->k, true, end, (size_t)std::min<int64_t>(opt->chunk_size + (opt->chunk_size >> 3) + 65536, (int64_t)1 << 31), sink);
	}
	if (ok) {
		const int64_t n_ins = yakamd_pass_end(h);
		if (n_ins < 0) ok = 0; else h->tot += (uint64_t)n_ins;   /* count.c:138 */
		if (ok && create_new && have_sid && yakamd_retained_instances(h) > 0) yk_ctx_set_source(((yak_ch_ext*)h)->ctx, sid, n_seq_tot);
	}
	fprintf(stderr, "[M::%s::%.3f*%.2f] %ld sequences in total; %ld distinct k-mers in the hash table\n", "yak_count",
	        yk_realtime(), yk_cputime() / (yk_realtime() + 1e-9), (long)n_seq_tot, (long)h->tot);
	if (getenv("YAKAMD_VERBOSE") && h) { (void)hipSetDevice(yk_ctx_device(((yak_ch_ext*)h)->ctx)); yk_pool_report("the pass"); }
	if (!ok) { if (!h0) yak_ch_destroy(h); return 0; }
	return h;
}

yak_ch_t *yak_count(const char *fn, const yak_copt_t *opt, yak_ch_t *h0) { return count_file(fn, opt, h0, false); }
yak_ch_t *yakamd_count_hpc(const char *fn, const yak_copt_t *opt, yak_ch_t *h0)
{
	if (h0 && !yakamd_ch_hpc(h0)) {
		yk_set_error("yakamd_count_hpc: the table is not marked as homopolymer-compressed (yakamd_ch_set_hpc); its keys were chosen in uncompressed space");
		return 0;
	}
	return count_file(fn, opt, h0, true);
}

/* reference count.c:168-193: clear the counts, then count the k-mers of fn that are in the table --
 * one count-existing pass on the device (sequences shorter than k have no k-mer either way) */
void yak_recount(const char *fn, yak_ch_t *h)
{
	yak_copt_t o;
	yak_copt_init(&o);
	o.k = h->k; o.pre = h->pre;
	/* count.c:172-173: an unreadable file leaves the table untouched.  (Asked, not tried: opening and closing a named pipe -- `yak recount <(zcat ...)` --
	 * would take the stream away from the count behind it) */
	if (fn != 0 && strcmp(fn, "-") != 0 && access(fn, R_OK) != 0) return;
	yak_ch_clear(h, 1);
	if (yak_count(fn, &o, h) == 0) fprintf(stderr, "[E::yak_recount] %s\n", yakamd_last_error());
}

} /* extern "C" */
