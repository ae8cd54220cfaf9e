/*
 * yak_lookup.cpp -- the lookup-only commands on the device: `yak qv` (reference qv.c), `yak triobin` (reference triobin.c),
 * `yak trioeval` (reference trioeval.c), `yak chkerr` (reference chkerr.c) and `yak sexchr` (reference sexchr.c).  The table is resident on
 * the device; every chunk of records is uploaded, its k-mers are looked up there (k_lookup) and reduced per record (k_qv_reduce, k_tb_reduce,
 * the k_te_* streak kernels, k_sc_reduce), and what the command prints comes from the values copied back.
 */
#include "yak_host.h"
#include "yak_amd.h"

namespace {

/* one chunk of records: every record, empty ones too, is a sequence of the image followed by '\n' (bseq.c:40 keeps records of any length) */
struct Chunk {
	std::vector<char> img;
	std::vector<uint64_t> off;
	std::vector<uint32_t> len;
	std::vector<std::string> names;            /* when the reader is asked for them */
	int64_t sum = 0;                           /* of the lengths */
	void clear() { img.clear(); off.clear(); len.clear(); names.clear(); sum = 0; }
	void add(const std::vector<char> &seq) { off.push_back(img.size()); len.push_back((uint32_t)seq.size()); img.insert(img.end(), seq.begin(), seq.end()); img.push_back('\n'); sum += (int64_t)seq.size(); }
	/* bseq.c:54: the chunk closes when the sum of the lengths reaches the chunk size; `max_bytes` bounds the image besides */
	bool full(int64_t chunk_size, size_t max_bytes) const { return sum >= chunk_size || img.size() > max_bytes; }
	/* the image padded with '\n' to a multiple of 16 bytes, as the device wants it; returns its length before */
	size_t pad() { const size_t nb = img.size(); img.resize((nb + 15) & ~(size_t)15, '\n'); return nb; }
};

/* the next chunk of `fx` (bseq.c:40-56); false when the input ended before the chunk was full */
bool read_chunk(FxReader &fx, int64_t chunk_size, size_t max_bytes, bool want_names, Chunk *ch)
{
	ch->clear();
	while (fx.next() >= 0) {
		if (want_names) ch->names.emplace_back(fx.name.begin(), fx.name.end());
		ch->add(fx.seq);
		if (ch->full(chunk_size, max_bytes)) return true;
	}
	return false;
}

/* a padded chunk's image, offsets and lengths on the device */
struct DevChunk {
	GrowBuf img, off, len;
	bool put(const Chunk &c) {
		const size_t ns = c.len.size();
		return img.fit(c.img.size()) && off.fit(ns * 8) && len.fit(ns * 4) && yakamd_memcpy_h2d(img.p, c.img.data(), c.img.size()) == 0
		       && yakamd_memcpy_h2d(off.p, c.off.data(), ns * 8) == 0 && yakamd_memcpy_h2d(len.p, c.len.data(), ns * 4) == 0;
	}
};

/* reference triobin.c:103-121, restated on c[] = the flag histogram (flag = pat class | mat class << 2) and sc[] = the
 * solid-run sums.  The operands keep the reference's order and types, so the double products round as there */
char tb_classify(const int32_t *c, const int32_t *sc, int k, double ratio)
{
	const int pat = c[2], mat = c[8];                /* c[0<<2|2], c[2<<2|0] */
	if (sc[0] == 0 && sc[1] == 0) {
		if (pat == mat) return '0';
		if (pat >= k - 4 + mat && (mat <= 1 || pat * 0.05 > mat)) return 'p';
		if (mat >= k - 4 + pat && (pat <= 1 || mat * 0.05 > pat)) return 'm';
		return '0';
	}
	if (sc[0] > k && sc[1] > k) return 'a';
	if (sc[0] >= k - 4 + sc[1] && sc[0] * 0.05 >= sc[1] && pat * ratio > mat) return 'p';
	if (sc[1] >= k - 4 + sc[0] && sc[1] * 0.05 >= sc[0] && mat * ratio > pat) return 'm';
	return 'a';
}

/* the lines a command writes, gathered and written out when 1 MiB has come together (drain) and after every chunk (flush); after a failed write
 * nothing more is written */
struct LineOut {
	std::string s;
	FILE *fp = 0;
	bool ok = true;
	void append(const char *t) { s += t; }
	void append(const std::string &t) { s += t; }
	void appendf(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
		char buf[256];
		va_list ap;
		va_start(ap, fmt);
		s.append(buf, (size_t)vsnprintf(buf, sizeof buf, fmt, ap));
		va_end(ap);
	}
	void drain() { if (s.size() >= (1u << 20)) flush(); }
	void flush() { ok = ok && fwrite(s.data(), 1, s.size(), fp) == s.size(); s.clear(); }
};

/* body(index of the input, chunk, the chunk on the device, length of its image before padding, out): the command's lookup, reduction and lines;
 * false after a device error */
typedef std::function<bool(int, const Chunk&, const DevChunk&, size_t, LineOut&)> ChunkBody;

/* What triobin, trioeval, chkerr and sexchr share: every input in turn is read in chunks of `chunk_size` bases (bseq.c:54), each chunk uploaded and
 * handed to `body`; the output (out_fn, or stdout) is `header`, body's lines, and what `tail` adds after the last chunk.  The next chunk is read on
 * a second thread while the device and the writer work on this one (the reference's two-step kt_pipeline).  -1 after a message when an input or the
 * output cannot be opened, a chunk fails (nothing from that chunk on is written) or a write fails */
int run_chunks(const char *who, std::initializer_list<const char*> fns, const char *out_fn, int64_t chunk_size, const char *header,
               const ChunkBody &body, const std::function<void(LineOut&)> &tail = nullptr)
{
	std::vector<FxReader> fx(fns.size());
	auto close_all = [&]() { for (FxReader &f : fx) f.close_file(); };
	size_t n_open = 0;
	for (const char *fn : fns)                                       /* every input before the output is created */
		if (!fx[n_open++].open_file(fn)) { fprintf(stderr, "[E::%s] cannot open '%s'\n", who, fn ? fn : "-"); close_all(); return -1; }
	LineOut out;
	out.fp = out_fn ? fopen(out_fn, "wb") : stdout;
	if (!out.fp) { fprintf(stderr, "[E::%s] cannot write '%s'\n", who, out_fn); close_all(); return -1; }
	if (chunk_size < 1) chunk_size = 1;
	out.s = header;
	DevChunk d;
	Chunk cur, nxt;
	bool ok = true;
	for (size_t f = 0; ok && f < fx.size(); ++f) {
		read_chunk(fx[f], chunk_size, SIZE_MAX, true, &cur);
		while (ok && !cur.len.empty()) {
			std::thread reader([&]() { read_chunk(fx[f], chunk_size, SIZE_MAX, true, &nxt); });
			fprintf(stderr, "[M::%s] read %ld sequences\n", who, (long)cur.len.size());
			const size_t nb = cur.pad();
			ok = d.put(cur) && body((int)f, cur, d, nb, out) && out.ok;
			if (ok) { out.flush(); ok = out.ok; }
			reader.join();                                           /* nxt is the reader's until here, whatever became of this chunk */
			std::swap(cur, nxt);
		}
		cur.clear();
	}
	if (ok) {
		if (tail) tail(out);
		out.flush();
		ok = out.ok;
	}
	if (!ok) fprintf(stderr, "[E::%s] %s\n", who, yakamd_last_error());
	if (out_fn) { if (fclose(out.fp) != 0) ok = false; }
	else fflush(out.fp);
	close_all();
	return ok ? 0 : -1;
}

/* a table in homopolymer-compressed space (yakamd_ch_set_hpc) looked up with uncompressed sequence answers wrongly without a sign:
 * the commands that have no compressed form refuse it before they create any output */
bool hpc_refuse(const yak_ch_t *ch, const char *who)
{
	if (!yakamd_ch_hpc(ch)) return false;
	yk_set_error("%s: the table is marked as homopolymer-compressed (yakamd_ch_set_hpc) and this command reads uncompressed sequence: only yak_qv() compresses what it looks up", who);
	return true;
}

}   // namespace

/* reference qv.c:137-144 */
void yak_qopt_init(yak_qopt_t *opt)
{
	memset(opt, 0, sizeof(yak_qopt_t));
	opt->chunk_size = 1000000000;
	opt->n_threads = 4;
	opt->min_frac = 0.5;
	opt->fpr = 0.00004;
}

/* reference qv.c:34-135.  Every chunk of sequences is looked up (k_lookup), reduced per sequence and binned (k_qv_reduce).  A chunk
 * also closes when its image exceeds 2^31 bytes.  The EK / SQ lines of -E / -p are printed from the values copied back, in input
 * order (the reference prints them in a thread-dependent order).  On a device error the function prints a message and leaves cnt zeroed. */
void yak_qv(const yak_qopt_t *opt, const char *fn, const yak_ch_t *ch, int64_t *cnt)
{
	const int n_cnt = 1 << YAK_COUNTER_BITS;
	memset(cnt, 0, n_cnt * sizeof(int64_t));
	yak_ch_t *h = (yak_ch_t*)ch;
	if (ch->k >= 32) { fprintf(stderr, "[E::yak_qv] k must be below 32\n"); return; }   /* qv.c:44 asserts */
	if (multi_refuse(ch, __func__)) return;                      /* the lookup kernel reads one table image: restore the .yak file for qv */
	const bool want_names = opt->print_each || opt->print_err_kmer;
	/* without -p / -E nothing of a record but its bases is needed: a plain, block-gzipped or gzip file then goes through the parallel reader
	 * (every record's sequence + '\n', in order: qv.c:45 skips the short ones later); with them the records are read one by one */
	SeqInput in;
	if (!in.open(fn, want_names ? 1 : parse_threads(opt->n_threads), 1 << 20)) return;
	const size_t max_bytes = (size_t)1 << 31;
	uint64_t *d_hist = (uint64_t*)yakamd_dev_alloc(n_cnt * 8);
	std::vector<uint64_t> zero(n_cnt, 0);
	std::vector<uint32_t> h_tot, h_non0;
	std::vector<unsigned short> h_t;
	Chunk chunk;
	DevChunk d;
	GrowBuf d_t, d_tot, d_non0, d_cimg, d_coff, d_clen;
	std::vector<uint64_t> c_off;                                 /* a marked table: the chunk's offsets and lengths in its compressed image */
	std::vector<uint32_t> c_len;
	const bool hpc = yakamd_ch_hpc(ch) != 0;
	bool ok = d_hist && yakamd_memcpy_h2d(d_hist, zero.data(), n_cnt * 8) == 0;
	auto flush = [&]() {
		const size_t ns = chunk.len.size();
		if (ns == 0) return;
		const size_t nb = chunk.pad();
		ok = ok && d.put(chunk) && d_t.fit(chunk.img.size() * 2) && d_tot.fit(ns * 4) && d_non0.fit(ns * 4);
		const void *img = d.img.p, *off = d.off.p, *len = d.len.p;
		int64_t n_img = (int64_t)nb;
		const uint64_t *h_off = chunk.off.data();
		const uint32_t *h_len = chunk.len.data();
		if (ok && hpc) {
			/* the table's k-mers are those of compressed sequence: the chunk is compacted on the device and everything behind -- the
			 * lookup, min_len, the SQ lengths and the EK positions -- is in compressed coordinates, as a run on the host-compressed file gives them */
			ok = d_cimg.fit(chunk.img.size()) && d_coff.fit(ns * 8) && d_clen.fit(ns * 4);
			if (ok) n_img = yakamd_hpc_dev(d.img.p, (int64_t)nb, d_cimg.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, (uint64_t*)d_coff.p, (uint32_t*)d_clen.p, 0);
			ok = ok && n_img >= 0;
			img = d_cimg.p; off = d_coff.p; len = d_clen.p;
			if (ok && want_names) {
				c_off.resize(ns); c_len.resize(ns);
				ok = yakamd_memcpy_d2h(c_off.data(), d_coff.p, ns * 8) == 0 && yakamd_memcpy_d2h(c_len.data(), d_clen.p, ns * 4) == 0;
				h_off = c_off.data(); h_len = c_len.data();
			}
		}
		ok = ok && yakamd_lookup_dev(h, img, n_img, d_t.p) == 0
		     && yakamd_qv_reduce_dev(h, d_t.p, (const uint64_t*)off, (const uint32_t*)len, (int64_t)ns, opt->min_len, opt->min_frac,
		                             (uint32_t*)d_tot.p, (uint32_t*)d_non0.p, d_hist) == 0;
		if (ok && want_names) {
			h_tot.resize(ns); h_non0.resize(ns);
			ok = yakamd_memcpy_d2h(h_tot.data(), d_tot.p, ns * 4) == 0 && yakamd_memcpy_d2h(h_non0.data(), d_non0.p, ns * 4) == 0;
			if (ok && opt->print_err_kmer) { h_t.resize(chunk.img.size()); ok = yakamd_memcpy_d2h(h_t.data(), d_t.p, chunk.img.size() * 2) == 0; }
			for (size_t j = 0; ok && j < ns; ++j) {
				if (h_tot[j] == 0xffffffffu) continue;                          /* below min_len: qv.c:45 */
				if (opt->print_err_kmer)
					for (uint32_t i = 0; i < h_len[j]; ++i)
						if (h_t[h_off[j] + i] == 0) printf("EK\t%s\t%d\n", chunk.names[j].c_str(), (int)(i + 1 - ch->k));
				if (opt->print_each) {
					const int tot = (int)h_tot[j], non0 = (int)h_non0[j];
					double qv = -1.0;
					if (tot > 0) {
						if (non0 > 0) {
							if (tot > non0) { qv = log((double)tot / non0) / ch->k; qv = -4.3429448190325175 * log(qv); }
							else qv = 99.0;
						} else qv = 0.0;
					}
					printf("SQ\t%s\t%d\t%d\t%d\t%.2f\n", chunk.names[j].c_str(), (int)h_len[j], tot, non0, qv);
				}
			}
		}
		fprintf(stderr, "[M::%s] processed %ld sequences\n", "yak_qv", (long)ns);
		chunk.clear();
	};
	const bool parallel = ok && in.kind != SeqInput::STREAM;
	if (parallel) {
		const ImgSink sink = [&](const char *img, size_t n, int64_t, const WinPack*) {
			const size_t base = chunk.img.size();
			for (const char *p = img, *e = img + n; p < e; ) {
				const char *q = (const char*)memchr(p, '\n', (size_t)(e - p));
				if (!q) q = e;
				chunk.off.push_back(base + (size_t)(p - img)); chunk.len.push_back((uint32_t)(q - p));
				chunk.sum += q - p;
				p = q + 1;
			}
			chunk.img.insert(chunk.img.end(), img, img + n);
			if (chunk.full(opt->chunk_size, max_bytes)) flush();
			return ok;
		};
		ok = in.run(0, false, sink) && ok;
	}
	for (bool more = !parallel; ok && more; ) {
		more = read_chunk(in.fx, opt->chunk_size, max_bytes, want_names, &chunk);
		flush();
	}
	if (ok) flush();                                             /* the parallel reader's last chunk */
	std::vector<uint64_t> hh(n_cnt, 0);
	ok = ok && yakamd_memcpy_d2h(hh.data(), d_hist, n_cnt * 8) == 0;
	if (ok) for (int i = 0; i < n_cnt; ++i) cnt[i] = (int64_t)hh[i];
	else fprintf(stderr, "[E::yak_qv] %s\n", yakamd_last_error());
	yakamd_dev_free(d_hist);
}

/* reference triobin.c:153-160 */
void yakamd_tbopt_init(yakamd_tbopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_tbopt_t));
	opt->ratio_thres = 0.33;
	opt->print_diff = 0;
	opt->n_threads = 8;
	opt->chunk_size = 200000000;
}

/* reference triobin.c:123-197 with one device and -t1's output order: per chunk, the D lines of -p (triobin.c:89-90) of every
 * read in input order, then one line per read (triobin.c:144-145).  A chunk closes on the sum of the lengths alone: the D lines
 * are printed per chunk. */
int yakamd_triobin(const yakamd_tbopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const int k = ch->k;
	if (hpc_refuse(ch, __func__)) return -1;
	GrowBuf d_flag, d_cnt;
	std::vector<uint8_t> flag;
	std::vector<int32_t> cnt;
	return run_chunks(__func__, { fn }, out_fn, opt->chunk_size, "", [&](int, const Chunk &cur, const DevChunk &d, size_t nb, LineOut &out) {
		const size_t ns = cur.len.size();
		cnt.resize(ns * 19);
		bool ok = d_flag.fit(nb) && d_cnt.fit(ns * 19 * 4)
		          && yakamd_triobin_lookup_dev(h, d.img.p, (int64_t)nb, d_flag.p) == 0
		          && yakamd_triobin_reduce_dev(k, d_flag.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, (int32_t*)d_cnt.p, 0) == 0
		          && yakamd_memcpy_d2h(cnt.data(), d_cnt.p, ns * 19 * 4) == 0;
		if (ok && opt->print_diff) {
			flag.resize(nb);
			ok = yakamd_memcpy_d2h(flag.data(), d_flag.p, nb) == 0;
			for (size_t j = 0; ok && out.ok && j < ns; ++j) {
				const uint8_t *f = flag.data() + cur.off[j];
				for (uint32_t i = 0; i < cur.len[j]; ++i) {
					const int v = f[i];
					if (v == 0xff || (v >> 2 & 3) == (v & 3)) continue;     /* no k-mer ends here, or both parents agree */
					out.append("D\t"); out.append(cur.names[j]);
					out.appendf("\t%u\t%d\t%d\n", i, v & 3, v >> 2 & 3);
				}
				out.drain();
			}
		}
		for (size_t j = 0; ok && out.ok && j < ns; ++j) {
			const int32_t *c = cnt.data() + j * 19, *sc = c + 16;
			out.append(cur.names[j]);
			out.appendf("\t%c\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", tb_classify(c, sc, k, opt->ratio_thres), sc[0], sc[1], c[2], c[8], c[1], c[4], c[18], c[0]);
			out.drain();
		}
		return ok;
	});
}

/* reference trioeval.c:146-147 */
void yakamd_teopt_init(yakamd_teopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_teopt_t));
	opt->min_n = 2;
	opt->print_err = 0;
	opt->print_frag = 1;
	opt->n_threads = 8;
	opt->chunk_size = 1000000000;
}

/* reference trioeval.c:119-212 with one device and -t1's output order: the C header, then per chunk the F / E lines of every sequence in
 * input order (trioeval.c:101-116, from the ordered streak list) and one S line per sequence (trioeval.c:136-145), then the W / H / N
 * lines.  A chunk closes where bseq_read(fp, 1000000000) closes it. */
int yakamd_trioeval(const yakamd_teopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const int k = ch->k;
	const bool want_list = opt->print_err || opt->print_frag;
	if (hpc_refuse(ch, __func__)) return -1;
	const char *header =
		"C\tS  seqName     #patKmer  #matKmer  #pat-pat  #pat-mat  #mat-pat  #mat-mat  seqLen\n"
		"C\tF  seqName     type      startPos  endPos    count\n"
		"C\tW  #switchErr  denominator  switchErrRate\n"
		"C\tH  #hammingErr denominator  hammingErrRate\n"
		"C\tN  #totPatKmer #totMatKmer  errRate\n"
		"C\n";
	int64_t n_pair = 0, n_site = 0, n_switch = 0, n_err = 0, n_par[2] = { 0, 0 };
	GrowBuf d_flag, d_cnt;
	std::vector<int32_t> cnt;
	std::vector<yakamd_streak_t> sk;
	return run_chunks(__func__, { fn }, out_fn, opt->chunk_size, header, [&](int, const Chunk &cur, const DevChunk &d, size_t nb, LineOut &out) {
		const size_t ns = cur.len.size();
		cnt.resize(ns * 6);
		void *d_sk = 0;
		int64_t n_sk = 0;
		bool ok = d_flag.fit(nb) && d_cnt.fit(ns * 6 * 4)
		          && yakamd_triobin_lookup_dev(h, d.img.p, (int64_t)nb, d_flag.p) == 0
		          && yakamd_trioeval_reduce_dev(k, opt->min_n, d_flag.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, (int64_t)nb,
		                                        (int32_t*)d_cnt.p, want_list ? &d_sk : 0, &n_sk, 0) == 0
		          && yakamd_memcpy_d2h(cnt.data(), d_cnt.p, ns * 6 * 4) == 0;
		sk.resize(want_list ? (size_t)n_sk : 0);
		if (ok && want_list && n_sk > 0) ok = yakamd_memcpy_d2h(sk.data(), d_sk, (size_t)n_sk * sizeof(yakamd_streak_t)) == 0;
		yakamd_dev_free(d_sk);
		if (ok && want_list) {                                    /* trioeval.c:101-116 per sequence, in input order */
			uint32_t seq = UINT32_MAX, last = 0, f_type = 0;
			int f_st = 0, f_en = 0, f_cnt = 0;
			auto frag = [&]() {
				if (f_type > 0 && opt->print_frag) {
					out.append("F\t"); out.append(cur.names[seq]);
					out.appendf("\t%d\t%d\t%d\t%d\n", (int)f_type, f_st, f_en, f_cnt);
				}
			};
			for (int64_t i = 0; out.ok && i < n_sk; ++i) {
				const yakamd_streak_t &s = sk[i];
				if (s.seq != seq) { if (seq != UINT32_MAX) frag(); seq = s.seq; last = 0; f_type = 0; out.drain(); }
				if (last > 0 && opt->print_err && last != s.type) {
					out.append("E\t"); out.append(cur.names[seq]);
					out.appendf("\t%d\t%d\t%d\n", (int)s.en, (int)last, (int)s.type);
				}
				if (f_type != s.type) { frag(); f_type = s.type; f_st = (int)s.st + 1 - k; f_cnt = 0; }
				++f_cnt; f_en = (int)s.en + 1;
				last = s.type;
			}
			if (seq != UINT32_MAX) frag();
		}
		for (size_t j = 0; ok && out.ok && j < ns; ++j) {          /* trioeval.c:136-145 */
			const int32_t *dd = cnt.data() + j * 6, *c = dd + 2;
			n_par[0] += dd[0]; n_par[1] += dd[1];
			if (dd[0] + dd[1] >= 2) {
				n_pair += c[0] + c[1] + c[2] + c[3];
				n_switch += c[1] + c[2];
				n_site += dd[0] + dd[1];
				n_err += dd[0] < dd[1] ? dd[0] : dd[1];
			}
			out.append("S\t"); out.append(cur.names[j]);
			out.appendf("\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", dd[0], dd[1], c[0], c[1], c[2], c[3], (int)cur.len[j]);
			out.drain();
		}
		return ok;
	}, [&](LineOut &out) {                                         /* trioeval.c:207-209: the operands' order and types as there */
		out.appendf("W\t%ld\t%ld\t%.6f\n", (long)n_switch, (long)n_pair, (double)n_switch / n_pair);
		out.appendf("H\t%ld\t%ld\t%.6f\n", (long)n_err, (long)n_site, (double)n_err / n_site);
		out.appendf("N\t%ld\t%ld\t%.6f\n", (long)n_par[0], (long)n_par[1], (double)(n_par[0] < n_par[1] ? n_par[0] : n_par[1]) / (n_par[0] + n_par[1]));
	});
}

/* reference chkerr.c:104-106 */
void yakamd_ceopt_init(yakamd_ceopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_ceopt_t));
	opt->min_cnt = 3;
	opt->min_streak = 5;
	opt->n_threads = 8;
	opt->chunk_size = 1000000000;
}

/* reference chkerr.c:22-69 and 99-133 with one device and -t1's output order: per chunk, the streak lines of every sequence in input order.
 * Each chunk is looked up into one byte per position (yakamd_chkerr_lookup_dev: 1 = low) and its streaks listed in order
 * (yakamd_chkerr_streaks_dev).  With min_streak < 0, te_worker also prints its initial `streak = 0, last = -1` (chkerr.c:62-64 when the first
 * low k-mer is not at position 0, chkerr.c:67 when there is none): `name \t 1-k \t 0 \t 0` ahead of the sequence's streaks, unless its first
 * streak starts at position 0 (k = 1). */
int yakamd_chkerr(const yakamd_ceopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const int k = ch->k;
	if (multi_refuse(ch, __func__) || hpc_refuse(ch, __func__)) return -1;   /* the lookup kernel reads one table image */
	const bool phantom = opt->min_streak < 0;
	GrowBuf d_low;
	std::vector<yakamd_streak_t> sk;
	return run_chunks(__func__, { fn }, out_fn, opt->chunk_size, "", [&](int, const Chunk &cur, const DevChunk &d, size_t nb, LineOut &out) {
		const size_t ns = cur.len.size();
		void *d_sk = 0;
		int64_t n_sk = 0;
		bool ok = d_low.fit(nb) && yakamd_chkerr_lookup_dev(h, d.img.p, (int64_t)nb, opt->min_cnt, d_low.p) == 0
		          && yakamd_chkerr_streaks_dev(opt->min_streak, d_low.p, (const uint64_t*)d.off.p, (int64_t)ns, (int64_t)nb, &d_sk, &n_sk, 0) == 0;
		sk.resize((size_t)n_sk);
		if (ok && n_sk > 0) ok = yakamd_memcpy_d2h(sk.data(), d_sk, (size_t)n_sk * sizeof(yakamd_streak_t)) == 0;
		yakamd_dev_free(d_sk);
		for (size_t j = 0, i = 0; ok && out.ok && j < ns; ++j) {   /* the sequences in input order, each with its streaks */
			if (phantom && !(i < sk.size() && sk[i].seq == j && sk[i].st == 0)) { out.append(cur.names[j]); out.appendf("\t%d\t0\t0\n", 1 - k); }
			for (; i < sk.size() && sk[i].seq == j; ++i) {
				const yakamd_streak_t &s = sk[i];
				out.append(cur.names[j]);
				out.appendf("\t%d\t%d\t%d\n", (int)s.st + 1 - k, (int)s.en, (int)(s.en - s.st));
			}
			out.drain();
		}
		return ok;
	});
}

/* reference sexchr.c:113-114 and 13 */
void yakamd_scopt_init(yakamd_scopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_scopt_t));
	opt->n_threads = 8;
	opt->chunk_size = 1000000000;
}

/* reference sexchr.c:28-140 with one device and -t1's output order: the two C lines, then one S line per sequence of hap1, then of hap2.  Each
 * chunk is looked up into flags (yakamd_triobin_lookup_dev: the three SEXCHR loads OR 1, 2 and 4 into a count field) and tallied per sequence
 * (yakamd_sexchr_reduce_dev). */
int yakamd_sexchr(const yakamd_scopt_t *opt, const yak_ch_t *ch, const char *fn_hap1, const char *fn_hap2, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	if (multi_refuse(ch, __func__) || hpc_refuse(ch, __func__)) return -1;
	const char *header = "C\tS  seqName  originalHap  0  #k-mer  #sexchr  #sex1-specifc  #sex2-specific\nC\n";   /* sexchr.c:120-121, its spelling */
	GrowBuf d_flag, d_cnt;
	std::vector<uint64_t> cnt;
	return run_chunks(__func__, { fn_hap1, fn_hap2 }, out_fn, opt->chunk_size, header, [&](int file, const Chunk &cur, const DevChunk &d, size_t nb, LineOut &out) {
		const size_t ns = cur.len.size();
		cnt.resize(ns * 4);
		const bool ok = d_flag.fit(nb) && d_cnt.fit(ns * 32)
		                && yakamd_triobin_lookup_dev(h, d.img.p, (int64_t)nb, d_flag.p) == 0
		                && yakamd_sexchr_reduce_dev(d_flag.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, (int64_t)nb, (uint64_t*)d_cnt.p, 0) == 0
		                && yakamd_memcpy_d2h(cnt.data(), d_cnt.p, ns * 32) == 0;
		for (size_t j = 0; ok && out.ok && j < ns; ++j) {
			const uint64_t *c = cnt.data() + j * 4;
			out.append("S\t"); out.append(cur.names[j]);
			out.appendf("\t%d\t0\t%ld\t%ld\t%ld\t%ld\n", file + 1, (long)c[0], (long)c[1], (long)c[2], (long)c[3]);
			out.drain();
		}
		return ok;
	});
}

/* as yakamd_ceopt_init: the chunk is chkerr's */
void yakamd_dpopt_init(yakamd_dpopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_dpopt_t));
	opt->window = 0;
	opt->n_threads = 8;
	opt->chunk_size = 1000000000;
}

/* `yak-amd depth` (not in the reference): per chunk the lookup of chkerr's driver into one u16 per position (yakamd_lookup_dev),
 * then the windows' reduction in batches of at most 2^24 windows (yk_depth_batch), each batch's 24 bytes per window copied back and its lines
 * formatted here -- the output buffer stays bounded whatever the window is.  Refused before the output is created: what the lookup itself
 * would refuse at the first chunk (k >= 32, a sharded table, an open pass) and a negative window */
int yakamd_depth(const yakamd_dpopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const yak_ch_ext *e = (const yak_ch_ext*)ch;
	const int k = ch->k;
	const int64_t w = opt->window;
	if (k >= 32) { fprintf(stderr, "[E::%s] k = %d: k must be below 32 (reference qv.c:44)\n", __func__, k); return -1; }
	if (w < 0) { fprintf(stderr, "[E::%s] a window of %ld k-mer starts\n", __func__, (long)w); return -1; }
	if (multi_refuse(ch, __func__) || hpc_refuse(ch, __func__)) return -1;   /* the lookup kernel reads one table image */
	if (e->magic != EXT_MAGIC || !e->ctx) { fprintf(stderr, "[E::%s] not an engine table\n", __func__); return -1; }
	if (yk_ctx_in_pass(e->ctx)) { fprintf(stderr, "[E::%s] lookup during an open pass\n", __func__); return -1; }
	GrowBuf d_t, d_woff, d_win;
	std::vector<uint64_t> woff;
	std::vector<yakamd_win_t> win;
	const char *header = "#name\tstart\tend\tn_kmer\tn_present\tmean\tmedian\tmax\n";
	return run_chunks(__func__, { fn }, out_fn, opt->chunk_size, header, [&](int, const Chunk &cur, const DevChunk &d, size_t nb, LineOut &out) {
		const size_t ns = cur.len.size();
		woff.resize(ns + 1);
		woff[0] = 0;
		for (size_t j = 0; j < ns; ++j) woff[j + 1] = woff[j] + (w > 0 && cur.len[j] > 0 ? ((uint64_t)cur.len[j] + w - 1) / w : 1);
		const uint64_t n_win = woff[ns], batch = (uint64_t)yk_depth_batch_max();
		bool ok = d_t.fit(cur.img.size() * 2) && d_woff.fit((ns + 1) * 8) && d_win.fit((size_t)std::min(n_win, batch) * sizeof(yakamd_win_t))
		          && yakamd_memcpy_h2d(d_woff.p, woff.data(), (ns + 1) * 8) == 0 && yakamd_lookup_dev(h, d.img.p, (int64_t)nb, d_t.p) == 0;
		size_t j = 0;                                              /* the sequence of the window being printed */
		for (uint64_t g0 = 0; ok && out.ok && g0 < n_win; g0 += batch) {
			const uint64_t nw = std::min(batch, n_win - g0);
			win.resize(nw);
			ok = yk_depth_batch(k, w, d_t.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (const uint64_t*)d_woff.p, (int64_t)ns, (int64_t)nb, g0,
			                    (uint32_t)nw, d_win.p, 0) == 0
			     && (hipStreamSynchronize(0) == hipSuccess || yk_set_error("depth reduce: %s", hipGetErrorString(hipGetLastError())) == 0)
			     && yakamd_memcpy_d2h(win.data(), d_win.p, nw * sizeof(yakamd_win_t)) == 0;
			for (uint64_t g = g0; ok && out.ok && g < g0 + nw; ++g) {
				while (g >= woff[j + 1]) ++j;
				const yakamd_win_t &x = win[g - g0];
				const uint64_t L = cur.len[j], st = w > 0 ? (g - woff[j]) * (uint64_t)w : 0, en = w > 0 && st + (uint64_t)w < L ? st + (uint64_t)w : L;
				out.append(cur.names[j]);
				out.appendf("\t%llu\t%llu\t%u\t%u\t%.3f\t%u\t%u\n", (unsigned long long)st, (unsigned long long)en, x.n_kmer, x.n_present,
				            x.n_kmer ? (double)x.sum / x.n_kmer : 0.0, x.median, x.max);
				out.drain();
			}
		}
		return ok;
	});
}

/* the table, every sequence with count 1 .. 1023 k-mers, no filter; the chunk is chkerr's */
void yakamd_cvopt_init(yakamd_cvopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_cvopt_t));
	opt->lo = 1;
	opt->hi = 1023;
	opt->mask = -1;
	opt->n_threads = 8;
	opt->chunk_size = 1000000000;
}

/* `yak-amd cover` (not in the reference): per chunk the lookup of chkerr's driver into one u16 per position (yakamd_lookup_dev),
 * then the fused pass of kern_cover.inc (yakamd_cover_dev) into one cover byte per position, the tallies per sequence and, in FASTA mode with a
 * mask, the masked image; with -b the run finder of chkerr (yakamd_chkerr_streaks_dev) lists the runs of cover bytes.  Copied back are the tallies,
 * the runs and, in FASTA mode, the masked image -- never the cover bytes.  Refused before the output is created: what the lookup itself would
 * refuse at the first chunk (k >= 32, a sharded table, an open pass), a compressed table and options outside their ranges */
int yakamd_cover(const yakamd_cvopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const yak_ch_ext *e = (const yak_ch_ext*)ch;
	const int k = ch->k, lo = opt->lo, hi = opt->hi;
	const bool fasta = opt->mask >= 0, invert = opt->invert != 0;
	if (k >= 32) { fprintf(stderr, "[E::%s] k = %d: k must be below 32 (reference qv.c:44)\n", __func__, k); return -1; }
	if (lo < 0 || hi < lo || hi > 1023) { fprintf(stderr, "[E::%s] the counts %d:%d are not inside 0:1023\n", __func__, lo, hi); return -1; }
	if (!(opt->min_frac >= 0.0 && opt->min_frac <= 1.0)) { fprintf(stderr, "[E::%s] a covered fraction of %g is not inside [0, 1]\n", __func__, opt->min_frac); return -1; }
	if (opt->min_hit < 0) { fprintf(stderr, "[E::%s] a minimum of %ld hits\n", __func__, (long)opt->min_hit); return -1; }
	if (opt->mask > 2) { fprintf(stderr, "[E::%s] mask %d is none of none (0), soft (1) and hard (2)\n", __func__, (int)opt->mask); return -1; }
	if (multi_refuse(ch, __func__) || hpc_refuse(ch, __func__)) return -1;   /* the lookup kernel reads one table image */
	if (e->magic != EXT_MAGIC || !e->ctx) { fprintf(stderr, "[E::%s] not an engine table\n", __func__); return -1; }
	if (yk_ctx_in_pass(e->ctx)) { fprintf(stderr, "[E::%s] lookup during an open pass\n", __func__); return -1; }
	GrowBuf d_t, d_cov, d_masked, d_tally;
	std::vector<yakamd_cov_t> tally;
	std::vector<yakamd_streak_t> sk;
	std::vector<char> masked;
	int64_t n_seq = 0, n_sel = 0, sum_len = 0, sum_kmer = 0, sum_hit = 0, sum_cov = 0;
	char header[96];
	snprintf(header, sizeof header, "#cover\tk=%d\tlo=%d\thi=%d\n", k, lo, hi);
	return run_chunks(__func__, { fn }, out_fn, opt->chunk_size, fasta ? "" : header, [&](int, const Chunk &cur, const DevChunk &d, size_t nb, LineOut &out) {
		const size_t ns = cur.len.size(), room = cur.img.size();
		const int mask = fasta ? opt->mask : 0;
		void *d_sk = 0;
		int64_t n_sk = 0;
		tally.resize(ns);
		bool ok = d_t.fit(room * 2) && d_cov.fit(room) && (mask == 0 || d_masked.fit(room)) && d_tally.fit(ns * sizeof(yakamd_cov_t))
		          && yakamd_lookup_dev(h, d.img.p, (int64_t)nb, d_t.p) == 0
		          && yakamd_cover_dev(k, lo, hi, d_t.p, (int64_t)nb, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, d.img.p, mask, d_cov.p,
		                              mask ? d_masked.p : 0, (yakamd_cov_t*)d_tally.p, 0) == 0
		          && yakamd_memcpy_d2h(tally.data(), d_tally.p, ns * sizeof(yakamd_cov_t)) == 0;
		if (ok && !fasta && opt->intervals) {
			ok = yakamd_chkerr_streaks_dev(-1, d_cov.p, (const uint64_t*)d.off.p, (int64_t)ns, (int64_t)nb, &d_sk, &n_sk, 0) == 0;
			sk.resize(ok ? (size_t)n_sk : 0);
			if (ok && n_sk > 0) ok = yakamd_memcpy_d2h(sk.data(), d_sk, (size_t)n_sk * sizeof(yakamd_streak_t)) == 0;
			yakamd_dev_free(d_sk);
		} else sk.clear();
		if (ok && mask) { masked.resize(nb); ok = yakamd_memcpy_d2h(masked.data(), d_masked.p, nb) == 0; }
		const char *bytes = mask ? masked.data() : cur.img.data();
		for (size_t j = 0, i = 0; ok && out.ok && j < ns; ++j) {   /* the sequences in input order, each with its runs */
			const yakamd_cov_t &x = tally[j];
			const bool sel = ((int64_t)x.n_hit >= opt->min_hit && (double)x.n_cov >= opt->min_frac * (double)cur.len[j]) != invert;
			++n_seq; n_sel += sel; sum_len += cur.len[j]; sum_kmer += x.n_kmer; sum_hit += x.n_hit; sum_cov += x.n_cov;
			if (sel && fasta) {
				out.append(">"); out.append(cur.names[j]); out.append("\n");
				out.s.append(bytes + cur.off[j], cur.len[j]);
				out.append("\n");
			} else if (sel) {
				out.append("S\t"); out.append(cur.names[j]);
				out.appendf("\t%u\t%u\t%u\t%u\t%u\n", cur.len[j], x.n_kmer, x.n_hit, x.n_cov, x.n_run);
			}
			for (; i < sk.size() && sk[i].seq <= j; ++i) {
				if (!sel || sk[i].seq != j) continue;
				out.append("B\t"); out.append(cur.names[j]);
				out.appendf("\t%u\t%u\n", sk[i].st, sk[i].en);
			}
			out.drain();
		}
		return ok;
	}, [&](LineOut &out) {
		if (!fasta) out.appendf("T\t%ld\t%ld\t%ld\t%ld\t%ld\t%ld\n", (long)n_seq, (long)n_sel, (long)sum_len, (long)sum_kmer, (long)sum_hit, (long)sum_cov);
	});
}
