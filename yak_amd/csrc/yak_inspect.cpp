/*
 * yak_inspect.cpp -- `yak inspect` (reference inspect.c) on the device.  The stored keys of in1 are streamed to the device in batches and
 * joined there with in2's table image (k_inspect, yakamd_inspect_dev) into the 1024 x 1024 histogram J[c0][c1] of inspect.c:56-60; the
 * lines are printed from J copied back.  yakamd_inspect_tables() runs the same join on two resident tables.
 */
#include "yak_host.h"
#include "yak_amd.h"
#include "yak_file.h"

namespace {

const int NC = YAK_N_COUNTS;

/* the header of a .yak file within inspect's limits: k in [1, 63], and pre up to 30 -- no table of in1 is built, its sub-tables are streamed; false after a message */
bool read_head(YakSrc &src, const char *fn, YakHeader *h)
{
	const YakStatus st = yak_read_header(src, h);
	if (st == YAK_SHORT_HEADER) { yk_set_error("inspect: '%s': truncated header", fn); return false; }
	if (st == YAK_BAD_MAGIC) { yk_set_error("inspect: '%s': wrong file magic", fn); return false; }
	if (st == YAK_BAD_BITS) { yk_set_error("inspect: '%s': saved counter bits %u, not %d", fn, h->bits, YAK_COUNTER_BITS); return false; }
	if (h->k < 1 || h->k > 63 || h->pre < YAK_COUNTER_BITS || h->pre > 30) { yk_set_error("inspect: '%s': k %u / pre %u out of range", fn, h->k, h->pre); return false; }
	return true;
}

/* the next batch of in1's body; false on a short read, after a message */
bool next_batch(YakBody &rd, const char *fn, int64_t cap, YakBatch *b)
{
	if (rd.next(cap, b) == YAK_OK) return true;
	yk_set_error("inspect: '%s': truncated at sub-table %d", fn, rd.cur);
	return false;
}

/* one batch on the device and joined into d_joint */
bool join_batch(const YakBatch &b, yak_ch_t *ch, int k, int pre, int ref_probe, GrowBuf &d_keys, GrowBuf &d_off, uint64_t *d_joint)
{
	if (b.keys.empty()) return true;
	const size_t nk = b.keys.size(), no = b.off.size();
	return d_keys.fit(nk * 8) && d_off.fit(no * 8) && yakamd_memcpy_h2d(d_keys.p, b.keys.data(), nk * 8) == 0
	       && yakamd_memcpy_h2d(d_off.p, b.off.data(), no * 8) == 0
	       && yakamd_inspect_dev(ch, k, pre, b.lo, b.lo + b.n_sub(), d_keys.p, (int64_t)nk, (const uint64_t*)d_off.p, 0, ref_probe, d_joint, 0) == 0;
}

/* the lines of inspect.c:64-101 from J (row c0), hist = yak_ch_hist of in2 (two tables) */
std::string format(const std::vector<int64_t> &J, const int64_t *hist, bool two, int max_cnt, int kmer)
{
	std::string out;
	char buf[64];
	std::vector<int64_t> tot(NC, 0);
	for (int i = 0; i < NC; ++i) { int64_t s = 0; for (int j = 0; j < NC; ++j) s += J[(size_t)i * NC + j]; tot[i] = s; }
	if (two) {
		const double fpr = 0.00004;
		int64_t acc_tot = 0, acc_cnt[NC];
		std::vector<int64_t> acc(J);
		for (int i = 0; i < NC; ++i) acc_cnt[i] = 0;
		for (int j = NC - 2; j >= 1; --j)
			for (int i = 0; i < NC; ++i) acc[(size_t)i * NC + j] += acc[(size_t)i * NC + (j + 1)];
		for (int i = NC - 1; i >= 0; --i) {
			acc_tot += tot[i];
			if (acc_tot == 0) continue;
			if (tot[i] == 0) continue;
			out.append(buf, (size_t)snprintf(buf, sizeof buf, "SN\t%d\t%ld\t%ld", i, (long)tot[i], (long)hist[i]));
			for (int j = 1; j <= max_cnt; ++j) {
				acc_cnt[j] += acc[(size_t)i * NC + j];
				out.append(buf, (size_t)snprintf(buf, sizeof buf, "\t%.4f", (double)acc_cnt[j] / acc_tot));
			}
			out += '\n';
		}
		acc = J;
		for (int i = NC - 2; i >= 0; --i)
			for (int j = 0; j < NC; ++j) acc[(size_t)i * NC + j] += acc[(size_t)(i + 1) * NC + j];
		yak_qstat_t *qs = (yak_qstat_t*)calloc(1, sizeof(yak_qstat_t));
		for (int i = max_cnt; i >= 1; --i) {
			if (tot[i] == 0) continue;
			yak_qv_solve(hist, &acc[(size_t)i * NC], kmer, fpr, qs);
			out.append(buf, (size_t)snprintf(buf, sizeof buf, "QV\t%d\t%ld\t%ld\t%.3f\t%.3f\n", i, (long)qs->tot, (long)acc[(size_t)i * NC], qs->qv_raw, qs->qv));
		}
		free(qs);
	} else {
		int64_t acc_tot = 0;
		for (int i = NC - 1; i >= 0; --i) {
			acc_tot += tot[i];
			if (acc_tot == 0) continue;
			out.append(buf, (size_t)snprintf(buf, sizeof buf, "HS\t%d\t%ld\t%ld\t%ld\n", i, (long)hist[i], (long)tot[i], (long)acc_tot));
		}
	}
	return out;
}

}   // namespace

void yakamd_inopt_init(yakamd_inopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_inopt_t));
	opt->max_cnt = 20;                                          /* inspect.c:11 */
	opt->ref_probe = 0;
	opt->n_threads = 4;
	opt->batch_keys = (int64_t)1 << 24;
}

/* reference inspect.c:8-105.  The checks of both headers come before any device call; the output is written only when everything succeeded */
int yakamd_inspect(const yakamd_inopt_t *opt, const char *fn1, const char *fn2, const char *out_fn)
{
	if (opt->max_cnt < 0 || opt->max_cnt > NC - 1) { yk_set_error("inspect: -m %d is outside [0, %d]", opt->max_cnt, NC - 1); return -1; }
	std::vector<char> fbuf((size_t)1 << 22);                    /* (outlives the stream) */
	FILE *fp = fopen(fn1, "rb");
	if (!fp) { yk_set_error("inspect: cannot open '%s'", fn1); return -1; }
	struct Closer { FILE *f; ~Closer() { fclose(f); } } fp_close{ fp };
	setvbuf(fp, fbuf.data(), _IOFBF, fbuf.size());
	YakSrc src = YakSrc::file(fp);
	YakHeader h1, h2;
	if (!read_head(src, fn1, &h1)) return -1;
	if (fn2) {
		FILE *f2 = fopen(fn2, "rb");
		if (!f2) { yk_set_error("inspect: cannot open '%s'", fn2); return -1; }
		YakSrc src2 = YakSrc::file(f2);
		const bool ok = read_head(src2, fn2, &h2);
		fclose(f2);
		if (!ok) return -1;
		if (h1.k != h2.k) { yk_set_error("inspect: the tables have different k (%d and %d)", (int)h1.k, (int)h2.k); return -1; }
		if (!opt->ref_probe && h1.k >= 32 && h1.pre != h2.pre) {
			yk_set_error("inspect: at k >= 32 a stored key holds hash bits [pre, pre + 54): the tables must have the same pre (%d and %d; -R probes as the reference does)", (int)h1.pre, (int)h2.pre);
			return -1;
		}
	}
	if (yakamd_device_count() < 1) { yk_set_error("inspect: no gfx950 GPU visible: inspect has no CPU path"); return -1; }
	const double t0 = yk_realtime();
	int64_t hist[NC];
	memset(hist, 0, sizeof hist);
	yak_ch_t *ch = 0;
	if (fn2) {
		ch = yak_ch_restore(fn2);
		if (!ch) { yk_set_error("inspect: cannot load '%s': %s", fn2, yakamd_last_error()); return -1; }
		yak_ch_hist(ch, hist, opt->n_threads);
	}
	const double t1 = yk_realtime();
	uint64_t *d_joint = (uint64_t*)yakamd_dev_alloc((size_t)NC * NC * 8);
	std::vector<int64_t> J((size_t)NC * NC, 0);
	bool ok = d_joint && yakamd_memcpy_h2d(d_joint, J.data(), J.size() * 8) == 0;
	YakBody rd(&src, (int)h1.pre);
	const int64_t cap = opt->batch_keys > 0 ? opt->batch_keys : 1;
	YakBatch cur, nxt;
	GrowBuf d_keys, d_off;
	double t_read = 0, t_join = 0;
	{
		const double a = yk_realtime();
		ok = ok && next_batch(rd, fn1, cap, &cur);
		t_read += yk_realtime() - a;
	}
	while (ok) {
		const bool more = !rd.done();
		bool rok = true;
		double t_rd = 0;
		std::thread reader;
		if (more) reader = std::thread([&]() { const double a = yk_realtime(); rok = next_batch(rd, fn1, cap, &nxt); t_rd = yk_realtime() - a; });
		const double a = yk_realtime();
		ok = join_batch(cur, ch, h1.k, h1.pre, opt->ref_probe, d_keys, d_off, d_joint);
		t_join += yk_realtime() - a;
		if (more) reader.join();
		t_read += t_rd;
		if (!ok) { fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error()); break; }
		if (!more) break;
		if (!rok) { ok = false; break; }
		std::swap(cur, nxt);
	}
	ok = ok && yakamd_memcpy_d2h(J.data(), d_joint, J.size() * 8) == 0;
	yakamd_dev_free(d_joint);
	yak_ch_destroy(ch);
	if (!ok) return -1;
	if (yak_verbose >= 3)
		fprintf(stderr, "[M::%s] %s: restore %.3f s, read %.3f s, join %.3f s (read overlaps the join)\n", __func__, fn2 ? "two tables" : "one table",
		        t1 - t0, t_read, t_join);
	const std::string text = format(J, hist, fn2 != 0, opt->max_cnt, h1.k);
	FILE *out = out_fn ? fopen(out_fn, "wb") : stdout;
	if (!out) { yk_set_error("inspect: cannot write '%s'", out_fn); return -1; }
	ok = fwrite(text.data(), 1, text.size(), out) == text.size();
	if (out_fn) { if (fclose(out) != 0) ok = false; }
	else fflush(out);
	return ok ? 0 : -1;
}

/* the join of yakamd_inspect on resident tables: A's keys in dump order come from its device-side .yak body (StagedRange), one rank's
 * sub-tables at a time, headers left in place */
int yakamd_inspect_tables(const yak_ch_t *a, const yak_ch_t *b, int ref_probe, int64_t *joint)
{
	std::vector<yakamd_ctx*> ea, eb;
	if (yk_inspect_engines(a, &ea) || (b && yk_inspect_engines(b, &eb))) { fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error()); return -1; }
	if (b && yk_ctx_device(ea[0]) != yk_ctx_device(eb[0])) {
		yk_set_error("inspect: the tables are on different devices (%d and %d)", yk_ctx_device(ea[0]), yk_ctx_device(eb[0]));
		return -1;
	}
	if (b && a->k != b->k) { yk_set_error("inspect: the tables have different k (%d and %d)", a->k, b->k); return -1; }
	if (b && !ref_probe && a->k >= 32 && a->pre != b->pre) {
		yk_set_error("inspect: at k >= 32 the tables must have the same pre (%d and %d)", a->pre, b->pre);
		return -1;
	}
	if (hipSetDevice(yk_ctx_device(ea[0])) != hipSuccess) { yk_set_error("inspect: cannot select device %d", yk_ctx_device(ea[0])); return -1; }
	uint64_t *d_joint = (uint64_t*)yakamd_dev_alloc((size_t)NC * NC * 8);
	std::vector<int64_t> J((size_t)NC * NC, 0);
	std::vector<TablePiece> pcs;
	bool ok = d_joint && yakamd_memcpy_h2d(d_joint, J.data(), J.size() * 8) == 0 && yk_table_pieces(a, 0, 1 << a->pre, "inspect", &pcs);
	StagedRange s;
	for (size_t i = 0; ok && i < pcs.size(); ++i)
		for (const TableRange &r : yk_ctx_ranges(pcs[i].c, pcs[i].lo, pcs[i].hi, INT64_MAX, false))   /* the piece as one range, if it holds keys */
			ok = ok && s.stage(pcs[i].c, r.lo, r.hi, &r.off, "inspect", "read") == 0
			     && yakamd_inspect_dev((yak_ch_t*)b, a->k, a->pre, r.lo, r.hi, s.d_img, (int64_t)r.n(), (const uint64_t*)s.off(), 1, ref_probe, d_joint, 0) == 0;
	s.drop();
	ok = ok && yakamd_memcpy_d2h(J.data(), d_joint, J.size() * 8) == 0;
	yakamd_dev_free(d_joint);
	if (!ok) { fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error()); return -1; }
	memcpy(joint, J.data(), J.size() * 8);
	return 0;
}
