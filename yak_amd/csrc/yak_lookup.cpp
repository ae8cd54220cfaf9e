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

/* a device buffer kept from one chunk to the next, grown when a chunk needs more */
struct DevBuf {
	void *p = 0;
	size_t cap = 0;
	bool fit(size_t n) { if (n <= cap) return true; yakamd_dev_free(p); cap = n + n / 8; p = yakamd_dev_alloc(cap); if (!p) cap = 0; return p != 0; }
	~DevBuf() { yakamd_dev_free(p); }
};

/* a padded chunk's image, offsets and lengths on the device */
struct DevChunk {
	DevBuf img, off, len;
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
	FxReader fx;
	if (!fx.open_file(fn)) return;
	const bool want_names = opt->print_each || opt->print_err_kmer;
	const size_t max_bytes = (size_t)1 << 31;
	uint64_t *d_hist = (uint64_t*)yakamd_dev_alloc(n_cnt * 8);
	std::vector<uint64_t> zero(n_cnt, 0);
	std::vector<uint32_t> h_tot, h_non0;
	std::vector<unsigned short> h_t;
	Chunk chunk;
	DevChunk d;
	DevBuf d_t, d_tot, d_non0;
	bool ok = d_hist && yakamd_memcpy_h2d(d_hist, zero.data(), n_cnt * 8) == 0;
	auto flush = [&]() {
		const size_t ns = chunk.len.size();
		if (ns == 0) return;
		const size_t nb = chunk.pad();
		ok = ok && d.put(chunk) && d_t.fit(chunk.img.size() * 2) && d_tot.fit(ns * 4) && d_non0.fit(ns * 4)
		     && yakamd_lookup_dev(h, d.img.p, (int64_t)nb, d_t.p) == 0
		     && yakamd_qv_reduce_dev(h, d_t.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, opt->min_len, opt->min_frac,
		                             (uint32_t*)d_tot.p, (uint32_t*)d_non0.p, d_hist) == 0;
		if (ok && want_names) {
			h_tot.resize(ns); h_non0.resize(ns);
			ok = yakamd_memcpy_d2h(h_tot.data(), d_tot.p, ns * 4) == 0 && yakamd_memcpy_d2h(h_non0.data(), d_non0.p, ns * 4) == 0;
			if (ok && opt->print_err_kmer) { h_t.resize(chunk.img.size()); ok = yakamd_memcpy_d2h(h_t.data(), d_t.p, chunk.img.size() * 2) == 0; }
			for (size_t j = 0; ok && j < ns; ++j) {
				if (h_tot[j] == 0xffffffffu) continue;                          /* below min_len: qv.c:45 */
				if (opt->print_err_kmer)
					for (uint32_t i = 0; i < chunk.len[j]; ++i)
						if (h_t[chunk.off[j] + i] == 0) printf("EK\t%s\t%d\n", chunk.names[j].c_str(), (int)(i + 1 - ch->k));
				if (opt->print_each) {
					const int tot = (int)h_tot[j], non0 = (int)h_non0[j];
					double qv = -1.0;
					if (tot > 0) {
						if (non0 > 0) {
							if (tot > non0) { qv = log((double)tot / non0) / ch->k; qv = -4.3429448190325175 * log(qv); }
							else qv = 99.0;
						} else qv = 0.0;
					}
					printf("SQ\t%s\t%d\t%d\t%d\t%.2f\n", chunk.names[j].c_str(), (int)chunk.len[j], tot, non0, qv);
				}
			}
		}
		fprintf(stderr, "[M::%s] processed %ld sequences\n", "yak_qv", (long)ns);
		chunk.clear();
	};
	/* without -p / -E nothing of a record but its bases is needed: a plain, block-gzipped or gzip file then goes through the parallel reader
	 * (every record's sequence + '\n', in order: qv.c:45 skips the short ones later) */
	const int n_thr = parse_threads(opt->n_threads);
	ByteSource psrc; int psrc_fd = -1;
	pgz::Reader *gz_p = new pgz::Reader;
	struct GzDrop { pgz::Reader *p; ~GzDrop() { pgz::Reader *q = p; yk_reap_later([q]() { delete q; }); } } gz_drop{ gz_p };
	bool parallel = false;
	if (ok && !want_names) {
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
		if (parallel_source(fn, fx, n_thr, 1 << 20, &psrc, &psrc_fd)) { parallel = true; ok = parse_parallel(&psrc, 0, n_thr, sink) && ok; }
		else if (gz_source(fn, fx, n_thr, gz_p)) { parallel = true; ok = parse_gz(gz_p, 0, n_thr, sink) && ok; }
		if (psrc_fd >= 0) ::close(psrc_fd);
	}
	for (bool more = !parallel; ok && more; ) {
		more = read_chunk(fx, opt->chunk_size, max_bytes, want_names, &chunk);
		flush();
	}
	if (ok) flush();                                             /* the parallel reader's last chunk */
	std::vector<uint64_t> hh(n_cnt, 0);
	ok = ok && yakamd_memcpy_d2h(hh.data(), d_hist, n_cnt * 8) == 0;
	if (ok) for (int i = 0; i < n_cnt; ++i) cnt[i] = (int64_t)hh[i];
	else fprintf(stderr, "[E::yak_qv] %s\n", yakamd_last_error());
	yakamd_dev_free(d_hist);
	fx.close_file();
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
 * are printed per chunk.  The next chunk is read on a second thread while the device and the writer work on this one (the
 * reference's two-step kt_pipeline). */
int yakamd_triobin(const yakamd_tbopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const int k = ch->k;
	FxReader fx;
	if (!fx.open_file(fn)) { fprintf(stderr, "[E::%s] cannot open '%s'\n", __func__, fn ? fn : "-"); return -1; }
	FILE *out = out_fn ? fopen(out_fn, "wb") : stdout;
	if (!out) { fprintf(stderr, "[E::%s] cannot write '%s'\n", __func__, out_fn); fx.close_file(); return -1; }
	const int64_t chunk_size = opt->chunk_size > 0 ? opt->chunk_size : 1;
	DevChunk d;
	DevBuf d_flag, d_cnt;
	std::vector<uint8_t> flag;
	std::vector<int32_t> cnt;
	std::string line;
	Chunk cur, nxt;
	read_chunk(fx, chunk_size, SIZE_MAX, true, &cur);
	bool ok = true;
	while (ok && !cur.len.empty()) {
		std::thread reader([&]() { read_chunk(fx, chunk_size, SIZE_MAX, true, &nxt); });
		const size_t ns = cur.len.size();
		fprintf(stderr, "[M::%s] read %ld sequences\n", __func__, (long)ns);
		const size_t nb = cur.pad();
		cnt.resize(ns * 19);
		ok = d.put(cur) && d_flag.fit(nb) && d_cnt.fit(ns * 19 * 4)
		     && yakamd_triobin_lookup_dev(h, d.img.p, (int64_t)nb, d_flag.p) == 0
		     && yakamd_triobin_reduce_dev(k, d_flag.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, (int32_t*)d_cnt.p, 0) == 0
		     && yakamd_memcpy_d2h(cnt.data(), d_cnt.p, ns * 19 * 4) == 0;
		if (ok && opt->print_diff) {
			flag.resize(nb);
			ok = yakamd_memcpy_d2h(flag.data(), d_flag.p, nb) == 0;
			char buf[64];
			for (size_t j = 0; ok && j < ns; ++j) {
				const uint8_t *f = flag.data() + cur.off[j];
				for (uint32_t i = 0; i < cur.len[j]; ++i) {
					const int v = f[i];
					if (v == 0xff || (v >> 2 & 3) == (v & 3)) continue;     /* no k-mer ends here, or both parents agree */
					line += "D\t"; line += cur.names[j];
					line.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%u\t%d\t%d\n", i, v & 3, v >> 2 & 3));
				}
				if (line.size() >= (1u << 20)) { ok = fwrite(line.data(), 1, line.size(), out) == line.size(); line.clear(); }
			}
		}
		if (ok) {
			char buf[160];
			for (size_t j = 0; j < ns; ++j) {
				const int32_t *c = cnt.data() + j * 19, *sc = c + 16;
				line += cur.names[j];
				line.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%c\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", tb_classify(c, sc, k, opt->ratio_thres),
				                                  sc[0], sc[1], c[2], c[8], c[1], c[4], c[18], c[0]));
				if (line.size() >= (1u << 20)) { ok = fwrite(line.data(), 1, line.size(), out) == line.size(); line.clear(); if (!ok) break; }
			}
			ok = ok && fwrite(line.data(), 1, line.size(), out) == line.size();
			line.clear();
		}
		reader.join();
		std::swap(cur, nxt);
	}
	if (!ok) fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error());
	if (out_fn) { if (fclose(out) != 0) ok = false; }
	else fflush(out);
	fx.close_file();
	return ok ? 0 : -1;
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
 * lines.  A chunk closes where bseq_read(fp, 1000000000) closes it.  The next chunk is read on a second thread while the device and the
 * writer work on this one (the reference's two-step kt_pipeline). */
int yakamd_trioeval(const yakamd_teopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const int k = ch->k;
	FxReader fx;
	if (!fx.open_file(fn)) { fprintf(stderr, "[E::%s] cannot open '%s'\n", __func__, fn ? fn : "-"); return -1; }
	FILE *out = out_fn ? fopen(out_fn, "wb") : stdout;
	if (!out) { fprintf(stderr, "[E::%s] cannot write '%s'\n", __func__, out_fn); fx.close_file(); return -1; }
	const int64_t chunk_size = opt->chunk_size > 0 ? opt->chunk_size : 1;
	const bool want_list = opt->print_err || opt->print_frag;
	std::string line =
		"C\tS  seqName     #patKmer  #matKmer  #pat-pat  #pat-mat  #mat-pat  #mat-mat  seqLen\n"
		"C\tF  seqName     type      startPos  endPos    count\n"
		"C\tW  #switchErr  denominator  switchErrRate\n"
		"C\tH  #hammingErr denominator  hammingErrRate\n"
		"C\tN  #totPatKmer #totMatKmer  errRate\n"
		"C\n";
	int64_t n_pair = 0, n_site = 0, n_switch = 0, n_err = 0, n_par[2] = { 0, 0 };
	DevChunk d;
	DevBuf d_flag, d_cnt;
	std::vector<int32_t> cnt;
	std::vector<yakamd_streak_t> sk;
	Chunk cur, nxt;
	read_chunk(fx, chunk_size, SIZE_MAX, true, &cur);
	bool ok = true;
	auto drain = [&]() { if (line.size() >= (1u << 20)) { ok = ok && fwrite(line.data(), 1, line.size(), out) == line.size(); line.clear(); } };
	while (ok && !cur.len.empty()) {
		std::thread reader([&]() { read_chunk(fx, chunk_size, SIZE_MAX, true, &nxt); });
		const size_t ns = cur.len.size();
		fprintf(stderr, "[M::%s] read %ld sequences\n", __func__, (long)ns);
		const size_t nb = cur.pad();
		cnt.resize(ns * 6);
		void *d_sk = 0;
		int64_t n_sk = 0;
		ok = d.put(cur) && d_flag.fit(nb) && d_cnt.fit(ns * 6 * 4)
		     && yakamd_triobin_lookup_dev(h, d.img.p, (int64_t)nb, d_flag.p) == 0
		     && yakamd_trioeval_reduce_dev(k, opt->min_n, d_flag.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, (int64_t)nb,
		                                   (int32_t*)d_cnt.p, want_list ? &d_sk : 0, &n_sk, 0) == 0
		     && yakamd_memcpy_d2h(cnt.data(), d_cnt.p, ns * 6 * 4) == 0;
		sk.resize(want_list ? (size_t)n_sk : 0);
		if (ok && want_list && n_sk > 0) ok = yakamd_memcpy_d2h(sk.data(), d_sk, (size_t)n_sk * sizeof(yakamd_streak_t)) == 0;
		yakamd_dev_free(d_sk);
		if (ok && want_list) {                                    /* trioeval.c:101-116 per sequence, in input order */
			char buf[96];
			uint32_t seq = UINT32_MAX, last = 0, f_type = 0;
			int f_st = 0, f_en = 0, f_cnt = 0;
			auto frag = [&]() {
				if (f_type > 0 && opt->print_frag) {
					line += "F\t"; line += cur.names[seq];
					line.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%d\n", (int)f_type, f_st, f_en, f_cnt));
				}
			};
			for (int64_t i = 0; ok && i < n_sk; ++i) {
				const yakamd_streak_t &s = sk[i];
				if (s.seq != seq) { if (seq != UINT32_MAX) frag(); seq = s.seq; last = 0; f_type = 0; drain(); }
				if (last > 0 && opt->print_err && last != s.type) {
					line += "E\t"; line += cur.names[seq];
					line.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%d\t%d\t%d\n", (int)s.en, (int)last, (int)s.type));
				}
				if (f_type != s.type) { frag(); f_type = s.type; f_st = (int)s.st + 1 - k; f_cnt = 0; }
				++f_cnt; f_en = (int)s.en + 1;
				last = s.type;
			}
			if (seq != UINT32_MAX) frag();
		}
		if (ok) {
			char buf[160];
			for (size_t j = 0; j < ns; ++j) {                      /* trioeval.c:136-145 */
				const int32_t *dd = cnt.data() + j * 6, *c = dd + 2;
				n_par[0] += dd[0]; n_par[1] += dd[1];
				if (dd[0] + dd[1] >= 2) {
					n_pair += c[0] + c[1] + c[2] + c[3];
					n_switch += c[1] + c[2];
					n_site += dd[0] + dd[1];
					n_err += dd[0] < dd[1] ? dd[0] : dd[1];
				}
				line += "S\t"; line += cur.names[j];
				line.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", dd[0], dd[1], c[0], c[1], c[2], c[3], (int)cur.len[j]));
				drain();
				if (!ok) break;
			}
		}
		reader.join();
		std::swap(cur, nxt);
	}
	if (ok) {                                                     /* trioeval.c:207-209: the operands' order and types as there */
		char buf[256];
		line.append(buf, (size_t)snprintf(buf, sizeof buf, "W\t%ld\t%ld\t%.6f\n", (long)n_switch, (long)n_pair, (double)n_switch / n_pair));
		line.append(buf, (size_t)snprintf(buf, sizeof buf, "H\t%ld\t%ld\t%.6f\n", (long)n_err, (long)n_site, (double)n_err / n_site));
		line.append(buf, (size_t)snprintf(buf, sizeof buf, "N\t%ld\t%ld\t%.6f\n", (long)n_par[0], (long)n_par[1],
		                                  (double)(n_par[0] < n_par[1] ? n_par[0] : n_par[1]) / (n_par[0] + n_par[1])));
		ok = fwrite(line.data(), 1, line.size(), out) == line.size();
	}
	if (!ok) fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error());
	if (out_fn) { if (fclose(out) != 0) ok = false; }
	else fflush(out);
	fx.close_file();
	return ok ? 0 : -1;
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
 * streak starts at position 0 (k = 1).  The next chunk is read on a second thread while the device and the writer work on this one. */
int yakamd_chkerr(const yakamd_ceopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const int k = ch->k;
	if (multi_refuse(ch, __func__)) return -1;                  /* the lookup kernel reads one table image */
	FxReader fx;
	if (!fx.open_file(fn)) { fprintf(stderr, "[E::%s] cannot open '%s'\n", __func__, fn ? fn : "-"); return -1; }
	FILE *out = out_fn ? fopen(out_fn, "wb") : stdout;
	if (!out) { fprintf(stderr, "[E::%s] cannot write '%s'\n", __func__, out_fn); fx.close_file(); return -1; }
	const int64_t chunk_size = opt->chunk_size > 0 ? opt->chunk_size : 1;
	const bool phantom = opt->min_streak < 0;
	DevChunk d;
	DevBuf d_low;
	std::vector<yakamd_streak_t> sk;
	std::string line;
	Chunk cur, nxt;
	read_chunk(fx, chunk_size, SIZE_MAX, true, &cur);
	bool ok = true;
	char buf[64];
	const int nb_ph = snprintf(buf, sizeof buf, "\t%d\t0\t0\n", 1 - k);
	const std::string ph(buf, (size_t)nb_ph);
	while (ok && !cur.len.empty()) {
		std::thread reader([&]() { read_chunk(fx, chunk_size, SIZE_MAX, true, &nxt); });
		const size_t ns = cur.len.size();
		fprintf(stderr, "[M::%s] read %ld sequences\n", __func__, (long)ns);
		const size_t nb = cur.pad();
		void *d_sk = 0;
		int64_t n_sk = 0;
		ok = d.put(cur) && d_low.fit(nb) && yakamd_chkerr_lookup_dev(h, d.img.p, (int64_t)nb, opt->min_cnt, d_low.p) == 0
		     && yakamd_chkerr_streaks_dev(opt->min_streak, d_low.p, (const uint64_t*)d.off.p, (int64_t)ns, (int64_t)nb, &d_sk, &n_sk, 0) == 0;
		sk.resize((size_t)n_sk);
		if (ok && n_sk > 0) ok = yakamd_memcpy_d2h(sk.data(), d_sk, (size_t)n_sk * sizeof(yakamd_streak_t)) == 0;
		yakamd_dev_free(d_sk);
		for (size_t j = 0, i = 0; ok && j < ns; ++j) {             /* the sequences in input order, each with its streaks */
			if (phantom && !(i < sk.size() && sk[i].seq == j && sk[i].st == 0)) { line += cur.names[j]; line += ph; }
			for (; i < sk.size() && sk[i].seq == j; ++i) {
				const yakamd_streak_t &s = sk[i];
				line += cur.names[j];
				line.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%d\t%d\t%d\n", (int)s.st + 1 - k, (int)s.en, (int)(s.en - s.st)));
			}
			if (line.size() >= (1u << 20)) { ok = fwrite(line.data(), 1, line.size(), out) == line.size(); line.clear(); }
		}
		ok = ok && fwrite(line.data(), 1, line.size(), out) == line.size();
		line.clear();
		reader.join();
		std::swap(cur, nxt);
	}
	if (!ok) fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error());
	if (out_fn) { if (fclose(out) != 0) ok = false; }
	else fflush(out);
	fx.close_file();
	return ok ? 0 : -1;
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
 * (yakamd_sexchr_reduce_dev).  The next chunk is read on a second thread while the device and the writer work on this one. */
int yakamd_sexchr(const yakamd_scopt_t *opt, const yak_ch_t *ch, const char *fn_hap1, const char *fn_hap2, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	if (multi_refuse(ch, __func__)) return -1;
	FxReader fx[2];
	const char *fns[2] = { fn_hap1, fn_hap2 };
	for (int i = 0; i < 2; ++i)
		if (!fx[i].open_file(fns[i])) {
			fprintf(stderr, "[E::%s] cannot open '%s'\n", __func__, fns[i] ? fns[i] : "-");
			if (i) fx[0].close_file();
			return -1;
		}
	FILE *out = out_fn ? fopen(out_fn, "wb") : stdout;
	if (!out) { fprintf(stderr, "[E::%s] cannot write '%s'\n", __func__, out_fn); fx[0].close_file(); fx[1].close_file(); return -1; }
	const int64_t chunk_size = opt->chunk_size > 0 ? opt->chunk_size : 1;
	std::string line = "C\tS  seqName  originalHap  0  #k-mer  #sexchr  #sex1-specifc  #sex2-specific\nC\n";   /* sexchr.c:120-121, its spelling */
	DevChunk d;
	DevBuf d_flag, d_cnt;
	std::vector<uint64_t> cnt;
	Chunk cur, nxt;
	bool ok = true;
	char buf[128];
	for (int hap = 1; ok && hap <= 2; ++hap) {
		FxReader &f = fx[hap - 1];
		read_chunk(f, chunk_size, SIZE_MAX, true, &cur);
		while (ok && !cur.len.empty()) {
			std::thread reader([&]() { read_chunk(f, chunk_size, SIZE_MAX, true, &nxt); });
			const size_t ns = cur.len.size();
			fprintf(stderr, "[M::%s] read %ld sequences\n", __func__, (long)ns);
			const size_t nb = cur.pad();
			cnt.resize(ns * 4);
			ok = d.put(cur) && d_flag.fit(nb) && d_cnt.fit(ns * 32)
			     && yakamd_triobin_lookup_dev(h, d.img.p, (int64_t)nb, d_flag.p) == 0
			     && yakamd_sexchr_reduce_dev(d_flag.p, (const uint64_t*)d.off.p, (const uint32_t*)d.len.p, (int64_t)ns, (int64_t)nb, (uint64_t*)d_cnt.p, 0) == 0
			     && yakamd_memcpy_d2h(cnt.data(), d_cnt.p, ns * 32) == 0;
			for (size_t j = 0; ok && j < ns; ++j) {
				const uint64_t *c = cnt.data() + j * 4;
				line += "S\t"; line += cur.names[j];
				line.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%d\t0\t%ld\t%ld\t%ld\t%ld\n", hap, (long)c[0], (long)c[1], (long)c[2], (long)c[3]));
				if (line.size() >= (1u << 20)) { ok = fwrite(line.data(), 1, line.size(), out) == line.size(); line.clear(); }
			}
			reader.join();
			std::swap(cur, nxt);
		}
		cur.clear();
	}
	ok = ok && fwrite(line.data(), 1, line.size(), out) == line.size();
	if (!ok) fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error());
	if (out_fn) { if (fclose(out) != 0) ok = false; }
	else fflush(out);
	fx[0].close_file(); fx[1].close_file();
	return ok ? 0 : -1;
}
