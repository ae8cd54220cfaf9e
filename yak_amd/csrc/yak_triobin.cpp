/*
 * yak_triobin.cpp -- `yak triobin` (reference triobin.c) on the device: the k-mers of every read are looked
 * up in a table that holds both parents' classes (yak_ch_restore_core with YAK_LOAD_TRIOBIN1 / 2), reduced
 * per read on the device (k_tb_lookup, k_tb_reduce), and the read is classified on the host.
 */
#include "yak_host.h"
#include "yak_amd.h"

/* reference triobin.c:153-160 */
void yakamd_tbopt_init(yakamd_tbopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_tbopt_t));
	opt->ratio_thres = 0.33;
	opt->print_diff = 0;
	opt->n_threads = 8;
	opt->chunk_size = 200000000;
}

namespace {

/* one chunk of records, closed where bseq_read closes it (bseq.c:40-56): records are added until the sum of
 * their lengths reaches the chunk size; every record, empty ones too, is a sequence of the image followed by '\n' */
struct TbChunk {
	std::vector<char> img;
	std::vector<uint64_t> off;
	std::vector<uint32_t> len;
	std::vector<std::string> names;
	void clear() { img.clear(); off.clear(); len.clear(); names.clear(); }
};

void tb_read_chunk(FxReader &fx, int64_t chunk_size, TbChunk *ch)
{
	ch->clear();
	int64_t sum = 0, l;
	while ((l = fx.next()) >= 0) {
		ch->off.push_back(ch->img.size());
		ch->len.push_back((uint32_t)l);
		ch->names.emplace_back(fx.name.begin(), fx.name.end());
		ch->img.insert(ch->img.end(), fx.seq.begin(), fx.seq.end());
		ch->img.push_back('\n');
		sum += l;
		if (sum >= chunk_size) break;
	}
}

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

struct DevBuf {
	void *p = 0;
	size_t cap = 0;
	bool fit(size_t n) { if (n <= cap) return true; yakamd_dev_free(p); cap = n + n / 8; p = yakamd_dev_alloc(cap); if (!p) cap = 0; return p != 0; }
	~DevBuf() { yakamd_dev_free(p); }
};

}   // namespace

/* reference triobin.c:123-197 with one device and -t1's output order: per chunk, the D lines of -p (triobin.c:89-90) of every
 * read in input order, then one line per read (triobin.c:144-145).  The next chunk is read on a second thread while the device
 * and the writer work on this one (the reference's two-step kt_pipeline). */
int yakamd_triobin(const yakamd_tbopt_t *opt, const yak_ch_t *ch, const char *fn, const char *out_fn)
{
	yak_ch_t *h = (yak_ch_t*)ch;
	const int k = ch->k;
	FxReader fx;
	if (!fx.open_file(fn)) { fprintf(stderr, "[E::%s] cannot open '%s'\n", __func__, fn ? fn : "-"); return -1; }
	FILE *out = out_fn ? fopen(out_fn, "wb") : stdout;
	if (!out) { fprintf(stderr, "[E::%s] cannot write '%s'\n", __func__, out_fn); fx.close_file(); return -1; }
	const int64_t chunk_size = opt->chunk_size > 0 ? opt->chunk_size : 1;
	DevBuf d_img, d_flag, d_off, d_len, d_cnt;
	std::vector<uint8_t> flag;
	std::vector<int32_t> cnt;
	std::string line;
	TbChunk cur, nxt;
	tb_read_chunk(fx, chunk_size, &cur);
	bool ok = true;
	while (ok && !cur.len.empty()) {
		std::thread reader([&]() { tb_read_chunk(fx, chunk_size, &nxt); });
		const size_t ns = cur.len.size(), nb = cur.img.size();
		fprintf(stderr, "[M::%s] read %ld sequences\n", __func__, (long)ns);
		cur.img.resize((nb + 15) & ~(size_t)15, '\n');
		cnt.resize(ns * 19);
		ok = d_img.fit(cur.img.size()) && d_flag.fit(nb) && d_off.fit(ns * 8) && d_len.fit(ns * 4) && d_cnt.fit(ns * 19 * 4)
		     && yakamd_memcpy_h2d(d_img.p, cur.img.data(), cur.img.size()) == 0
		     && yakamd_memcpy_h2d(d_off.p, cur.off.data(), ns * 8) == 0 && yakamd_memcpy_h2d(d_len.p, cur.len.data(), ns * 4) == 0
		     && yakamd_triobin_lookup_dev(h, d_img.p, (int64_t)nb, d_flag.p) == 0
		     && yakamd_triobin_reduce_dev(k, d_flag.p, (const uint64_t*)d_off.p, (const uint32_t*)d_len.p, (int64_t)ns, (int32_t*)d_cnt.p, 0) == 0
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
