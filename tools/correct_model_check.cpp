/* correct_model_check.cpp -- the sequential model of the correction kernels (yak_amd/correct/correct.hip): the find, the trial
 * image and the decisions with the very functions of yak_amd/correct/correct_step.h, a position or a record at a time in image order, the texts of
 * correct_text.h and the reader of yak_amd/layer/seq_reader.h.  Host compiler only, built with the address and undefined-behaviour sanitizers
 * (tools/Makefile) and run as a program of its own by tests/test_correct_model.py.  The lookups are served from the stored keys of a .yak dump:
 *
 *   correct_model_check <table> <reads> <mode> [chunk_size]
 *
 * <table>: u32 k, min_cnt, min_run, u64 n, then n times (u64 canonical k-mer, u32 count), little endian.  <reads>: FASTA or FASTQ, plain or gzip.
 * <mode>: report (with its X lines) | reads | records (all reads as one image: a line per record, a line per tally) | trials (that image's trial
 * image, raw) | nt4 (the 256 codes of cr_nt4) | damage-at, damage-run, damage-p, damage-base (the first record damaged behind the find: the trials
 * must refuse it).  chunk_size: bases per chunk for report and reads [1 << 28].  Exit 1 with a message for what does not fit. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "../yak_amd/correct/correct_step.h"
#include "../yak_amd/correct/correct_text.h"
#include "../yak_amd/layer/seq_reader.h"

namespace {

struct Table {
	int k = 0, min_cnt = 0, min_run = 0;
	std::vector<std::pair<uint64_t, uint32_t>> keys;               /* ascending */
	uint32_t get(uint64_t x) const
	{
		const auto it = std::lower_bound(keys.begin(), keys.end(), std::make_pair(x, (uint32_t)0));
		return it != keys.end() && it->first == x ? it->second : 0;
	}
};

int die(const char *msg) { fprintf(stderr, "correct_model_check: %s\n", msg); return 1; }
bool put(const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, stdout) == n; }

bool load(const char *fn, Table *t)
{
	FILE *f = fopen(fn, "rb");
	if (!f) return false;
	uint32_t h[3];
	uint64_t n = 0;
	bool ok = fread(h, 4, 3, f) == 3 && fread(&n, 8, 1, f) == 1 && h[0] >= 1 && h[0] < 32 && n < ((uint64_t)1 << 32);
	t->k = (int)h[0]; t->min_cnt = (int)h[1]; t->min_run = (int)h[2];
	for (uint64_t i = 0; ok && i < n; ++i) {
		uint64_t x;
		uint32_t c;
		ok = fread(&x, 8, 1, f) == 1 && fread(&c, 4, 1, f) == 1;
		if (ok) t->keys.push_back(std::make_pair(x, c));
	}
	fclose(f);
	std::sort(t->keys.begin(), t->keys.end());
	return ok;
}

/* what yakamd_lookup_dev() writes for the image */
std::vector<uint16_t> lookup(const Table &t, const std::vector<uint8_t> &img)
{
	const int k = t.k;
	const uint64_t mask = ((uint64_t)1 << 2 * k) - 1;
	std::vector<uint16_t> out(img.size(), (uint16_t)CR_NONE);
	uint64_t fw = 0, rv = 0;
	int l = 0;
	for (size_t i = 0; i < img.size(); ++i) {
		const int c = cr_nt4(img[i]);
		if (c > 3) { l = 0; fw = rv = 0; continue; }
		fw = (fw << 2 | (uint64_t)c) & mask;
		rv = rv >> 2 | (uint64_t)(3 - c) << 2 * (k - 1);
		if (++l >= k) out[i] = (uint16_t)std::min<uint32_t>(t.get(std::min(fw, rv)), 1023);
	}
	return out;
}

struct WholeAt {                                                   /* the count array, CR_NONE outside it */
	const std::vector<uint16_t> *t;
	uint32_t operator()(int64_t i) const { return i < 0 || i >= (int64_t)t->size() ? (uint32_t)CR_NONE : (*t)[(size_t)i]; }
};
struct WholeBase {
	const std::vector<uint8_t> *b;
	uint8_t operator()(uint64_t g) const { return (*b)[(size_t)g]; }
};

struct Image {
	std::vector<uint8_t> img;
	std::vector<uint64_t> off;
	std::vector<uint32_t> len;
	std::vector<seq_record_t> recs;
	void clear() { img.clear(); off.clear(); len.clear(); recs.clear(); }
};

/* k_cor_find: a position at a time, in image order */
void find(const Table &t, const std::vector<uint16_t> &cnt, const Image &im, std::vector<cr_fix_t> *fix, std::vector<cr_tally_t> *tally)
{
	const WholeAt at{ &cnt };
	const int64_t n_seq = (int64_t)im.off.size();
	tally->assign(im.off.size(), cr_tally_t{ 0, 0, 0, 0, 0, 0, 0, 0 });
	for (int64_t i = 0; i < (int64_t)cnt.size(); ++i) {
		const uint32_t v = at(i);
		const int64_t s = cr_exists(v) ? cr_seq_of(im.off.data(), im.len.data(), 0, n_seq, (uint64_t)i) : -1;
		if (s < 0) continue;
		cr_tally_t &ts = (*tally)[(size_t)s];
		++ts.n_kmer;
		if (!cr_weak(v, (uint32_t)t.min_cnt)) continue;
		++ts.n_weak; ++ts.n_weak_after;
		if (cr_weak(at(i - 1), (uint32_t)t.min_cnt)) continue;
		uint32_t en = 0, p = 0;
		int run_len = 0;
		const uint32_t st = (uint32_t)((uint64_t)i - im.off[(size_t)s]);
		if (!cr_run(at, i, st, t.k, (uint32_t)t.min_cnt, t.min_run, &en, &p, &run_len)) continue;
		++ts.n_cand;
		cr_fix_t r;
		memset(&r, 0, sizeof r);
		r.at = im.off[(size_t)s] + p; r.seq = (uint32_t)s; r.p = p; r.st = st; r.en = en;
		fix->push_back(r);
	}
}

/* k_cor_trials: a record at a time.  false: a record does not fit */
bool trials(const Table &t, const Image &im, const std::vector<cr_fix_t> &fix, std::vector<uint8_t> *out)
{
	const int k = t.k;
	out->assign((6 * (size_t)k * fix.size() + 15) / 16 * 16, (uint8_t)'\n');
	const WholeBase base{ &im.img };
	for (size_t i = 0; i < fix.size(); ++i) {
		const int o = cr_rec_ok(&fix[i], k, im.img.size(), -1) ? cr_nt4(im.img[(size_t)fix[i].at]) : 4;
		if (o > 3) return false;
		for (int j = 0; j < 6 * k; ++j) (*out)[6 * (size_t)k * i + (size_t)j] = cr_trial_byte(base, &fix[i], k, o, j);
	}
	return true;
}

/* k_cor_decide: a record at a time */
bool decide(const Table &t, const std::vector<uint16_t> &tc, std::vector<cr_fix_t> *fix, Image *im, std::vector<cr_tally_t> *tally)
{
	const int k = t.k;
	const uint32_t c = (uint32_t)t.min_cnt;
	for (size_t i = 0; i < fix->size(); ++i) {
		cr_fix_t &r = (*fix)[i];
		if (!cr_rec_ok(&r, k, im->img.size(), (int64_t)tally->size())) return false;
		const uint8_t from = im->img[(size_t)r.at];
		const int o = cr_nt4(from);
		if (o > 3) return false;
		int fit = 0;
		for (int a = 0; a < 3; ++a) {
			bool all = true;
			for (int e = 0; e < (int)(r.en - r.st); ++e) {
				const uint32_t v = tc[(size_t)cr_trial_entry(i, a, k, e)];
				all = all && cr_exists(v) && !cr_weak(v, c);
			}
			if (all) fit |= 1 << cr_trial_code(o, a);
		}
		uint8_t to;
		const int why = cr_decide(fit, from, &to);
		r.from = from; r.to = to; r.fit = (uint8_t)fit; r.why = (uint8_t)why;
		cr_tally_t &ts = (*tally)[r.seq];
		if (why == CR_DONE) { ++ts.n_fixed; ts.n_weak_after -= r.en - r.st; im->img[(size_t)r.at] = to; }
		else if (why == CR_AMBIG) ++ts.n_ambig;
		else ++ts.n_nofit;
	}
	return true;
}

/* one image through the model, its lines behind the texts */
bool run_image(const Table &t, Image *im, std::string *report, std::string *reads, crt_total_t *tot)
{
	std::vector<cr_fix_t> fix;
	std::vector<cr_tally_t> tally;
	std::vector<uint8_t> tr;
	find(t, lookup(t, im->img), *im, &fix, &tally);
	if (!fix.empty()) {
		if (!trials(t, *im, fix, &tr) || !decide(t, lookup(t, tr), &fix, im, &tally)) return false;
	}
	size_t f = 0;
	for (size_t j = 0; j < im->recs.size(); ++j) {
		crt_seq(*report, im->recs[j].name, im->len[j], tally[j], tot);
		for (; f < fix.size() && fix[f].seq <= j; ++f) if (fix[f].seq == j && fix[f].why == CR_DONE) crt_fix(*report, im->recs[j].name, fix[f]);
		crt_read(*reads, im->recs[j].name, im->recs[j].comment, im->recs[j].qual, (const char*)im->img.data() + im->off[j], im->len[j]);
	}
	return true;
}

void add(Image *im, seq_record_t &r)
{
	im->off.push_back(im->img.size());
	im->len.push_back((uint32_t)r.seq.size());
	im->img.insert(im->img.end(), r.seq.begin(), r.seq.end());
	im->img.push_back((uint8_t)'\n');
	r.seq.clear();
	im->recs.push_back(r);
}

}   // namespace

int main(int argc, char **argv)
{
	if (argc < 4) return die("usage: correct_model_check <table> <reads> <mode> [chunk_size]");
	const std::string mode = argv[3];
	if (mode == "nt4") { for (int b = 0; b < 256; ++b) printf("%d\n", cr_nt4((uint8_t)b)); return 0; }
	Table t;
	if (!load(argv[1], &t)) return die("the table cannot be read");
	if (t.min_cnt < 1 || t.min_cnt > 1023 || t.min_run < 1 || t.min_run > t.k) return die("min_cnt or min_run out of range");
	const uint64_t chunk = argc > 4 ? strtoull(argv[4], 0, 10) : (uint64_t)1 << 28;
	if (chunk < 1) return die("chunk_size out of range");
	SeqReader rd(true);
	if (!rd.open(argv[2])) return die("the reads cannot be opened");
	Image im;
	seq_record_t r;
	if (mode == "report" || mode == "reads") {
		std::string report, reads;
		crt_total_t tot;
		memset(&tot, 0, sizeof tot);
		crt_head(report, t.k, t.min_cnt, t.min_run);
		uint64_t bases = 0;
		bool more = true;
		while (more) {
			more = rd.next(r);
			if (more) { bases += r.seq.size(); add(&im, r); }
			if ((!more || bases >= chunk) && !im.recs.empty()) {
				if (!run_image(t, &im, &report, &reads, &tot)) return die("a record does not fit");
				im.clear(); bases = 0;
			}
		}
		crt_last(report, tot);
		const std::string &out = mode == "report" ? report : reads;
		return put(out.data(), out.size()) ? 0 : die("cannot write");
	}
	while (rd.next(r)) add(&im, r);
	im.img.resize((im.img.size() + 15) / 16 * 16, (uint8_t)'\n');       /* as the command pads a chunk */
	std::vector<cr_fix_t> fix;
	std::vector<cr_tally_t> tally;
	std::vector<uint8_t> tr;
	find(t, lookup(t, im.img), im, &fix, &tally);
	if (mode.compare(0, 7, "damage-") == 0) {
		if (fix.empty()) return die("no record to damage");
		cr_fix_t &d = fix[0];
		if (mode == "damage-at") d.at = im.img.size();
		else if (mode == "damage-run") d.en = d.st + (uint32_t)t.k + 1;
		else if (mode == "damage-p") d.p = d.p + 1;
		else if (mode == "damage-base") d.at = im.off[d.seq] + im.len[d.seq];          /* the newline behind the sequence */
		else return die("no such damage");
	}
	if (!trials(t, im, fix, &tr)) return die("a record does not lie inside the image, or on a byte that is no base");
	if (mode == "trials") return put(tr.data(), tr.size()) ? 0 : die("cannot write");
	if (mode != "records") return die("no such mode");
	if (!decide(t, lookup(t, tr), &fix, &im, &tally)) return die("a record does not fit");
	for (const cr_fix_t &x : fix)
		printf("%llu %u %u %u %u %u %u %u %u\n", (unsigned long long)x.at, x.seq, x.p, x.st, x.en, x.from, x.to, x.fit, x.why);
	for (const cr_tally_t &s : tally) printf("t %u %u %u %u %u %u %u\n", s.n_kmer, s.n_weak, s.n_cand, s.n_fixed, s.n_ambig, s.n_nofit, s.n_weak_after);
	return 0;
}
