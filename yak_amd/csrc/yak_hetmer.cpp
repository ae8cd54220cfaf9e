/*
 * yak_hetmer.cpp -- `yak-amd hetmers` (not in the reference): the het-mer pairs of a count table, the k-mers that differ in
 * the middle base alone, as the 1024 x 1024 histogram J[lo][hi] of their two counts, the number of groups of 1 to 4 such k-mers, and the pairs
 * themselves.  The table's stored keys are staged in ranges of whole sub-tables (yk_ctx_dump_image_dev, the .yak body in listing order) of at most
 * batch_keys keys each, so the staging memory is bounded; every staged key probes the whole resident image for its three middle-base variants
 * (k_hetmer, kern_hetmer.inc), so a pair whose members lie in different ranges is found like any other.  No host mirror of the table is built.
 */
#include <string>
#include "engine_int.h"

namespace {

const int NC = YAK_N_COUNTS;
const int64_t HM_BATCH_DEFAULT = (int64_t)1 << 24;

/* the context a het-mer call works on, or 0 after a refusal (yk_whole_image_ctx) */
yakamd_ctx *hm_ctx(const yak_ch_t *h, int min_cnt, const char *what)
{
	return yk_whole_image_ctx(h, min_cnt, what, "the het-mer join has no CPU fallback", "a k-mer of even length has no middle base");
}

int64_t hm_batch(int64_t dflt)
{
	const int64_t b = yk_knob("YAKAMD_HETMER_BATCH", dflt);
	return b < 1 ? 1 : b;
}

/* a range of the table that holds keys, at most hm_batch() of them (table_ranges.h), staged with its offsets */
typedef TableRange Range;
int hm_stage(StagedRange &s, yakamd_ctx *c, const Range &r) { return s.stage(c, r.lo, r.hi, &r.off, "hetmers", "read"); }

/* the scratch of the pair list: the tiles' pair counts and their scan */
struct PairScratch {
	GrowBuf cnt, off;
	/* the pairs each tile of the staged range reports, scanned; *total = their number.  Returns when it is known */
	int count(yakamd_ctx *c, const Range &r, const StagedRange &s, int min_cnt, hipStream_t st, u64 *total)
	{
		const u64 nt = yk_hetmer_tiles(r.n());
		if (!cnt.fit(nt * 4) || !off.fit((nt + 1) * 8)) return fail("hetmers: no device memory for %llu tile counts", (unsigned long long)nt);
		if (yk_launch_hetmer(1, s.d_img, s.off(), r.n(), r.hi - r.lo, r.lo, min_cnt, img_view(c), 0, 0, (u32*)cnt.p, 0, 0, st))
			return fail("hetmers: the pair count did not launch");
		yk_launch_te_scan((const u32*)cnt.p, (int64_t)nt, 1, (u64*)off.p, st);
		HIPCK(hipGetLastError());
		HIPCK(hipMemcpyAsync(total, (const u64*)off.p + nt, 8, hipMemcpyDeviceToHost, st));
		HIPCK(hipStreamSynchronize(st));
		return 0;
	}
	/* after count(): the records into d_list[0 .. total).  Asynchronous on st */
	int write(yakamd_ctx *c, const Range &r, const StagedRange &s, int min_cnt, void *d_list, hipStream_t st)
	{
		if (yk_launch_hetmer(2, s.d_img, s.off(), r.n(), r.hi - r.lo, r.lo, min_cnt, img_view(c), 0, 0, 0, (const u64*)off.p, d_list, st))
			return fail("hetmers: the pair list did not launch");
		return 0;
	}
};

void kmer_text(char *s, u64 x, int k) { for (int j = 0; j < k; ++j) s[j] = "ACGT"[x >> 2 * (k - 1 - j) & 3]; }

}   // namespace

extern "C" int yakamd_hetmers_dev(yak_ch_t *h, int min_cnt, uint64_t *d_joint, uint64_t *d_group, void *stream)
{
	yakamd_ctx *c = hm_ctx(h, min_cnt, "hetmers");
	if (!c) return -1;
	if (!d_joint || !d_group || ((uintptr_t)d_joint & 7) != 0 || ((uintptr_t)d_group & 7) != 0) return fail("hetmers: the histogram and the group counts must be 8-byte aligned device arrays");
	HIPCK(hipSetDevice(c->dev));
	const hipStream_t st = (hipStream_t)stream;
	StagedRange s;
	for (const Range &r : yk_ctx_ranges(c, 0, c->P, hm_batch(HM_BATCH_DEFAULT), false)) {
		if (hm_stage(s, c, r)) return -1;
		if (yk_launch_hetmer(0, s.d_img, s.off(), r.n(), r.hi - r.lo, r.lo, min_cnt, img_view(c), (u64*)d_joint, (u64*)d_group, 0, 0, 0, st))
			return fail("hetmers: the join did not launch");
		HIPCK(hipStreamSynchronize(st));                             /* the staged keys go when the next range is staged, or with `s` */
	}
	return 0;
}

extern "C" int64_t yakamd_hetmer_pairs_dev(yak_ch_t *h, int min_cnt, void *d_pairs, int64_t cap)
{
	yakamd_ctx *c = hm_ctx(h, min_cnt, "hetmer pairs");
	if (!c) return -1;
	if (d_pairs && ((uintptr_t)d_pairs & 7) != 0) return fail("hetmer pairs: the records must be 8-byte aligned");
	HIPCK(hipSetDevice(c->dev));
	const std::vector<Range> ranges = yk_ctx_ranges(c, 0, c->P, hm_batch(HM_BATCH_DEFAULT), false);
	StagedRange s;
	PairScratch ps;
	/* the number first: nothing is written before it is known to fit */
	std::vector<u64> tot(ranges.size(), 0);
	u64 n = 0;
	for (size_t i = 0; i < ranges.size(); ++i) {
		if (hm_stage(s, c, ranges[i]) || ps.count(c, ranges[i], s, min_cnt, c->st, &tot[i])) return -1;
		n += tot[i];
	}
	if (!d_pairs || cap < (int64_t)n) return (int64_t)n;
	u64 at = 0;
	for (size_t i = 0; i < ranges.size(); ++i) {
		if (tot[i] == 0) continue;
		u64 again = 0;
		if (hm_stage(s, c, ranges[i]) || ps.count(c, ranges[i], s, min_cnt, c->st, &again)) return -1;
		if (again != tot[i]) return fail("hetmer pairs: the table changed while it was read");
		if (ps.write(c, ranges[i], s, min_cnt, (yakamd_hetpair_t*)d_pairs + at, c->st)) return -1;
		HIPCK(hipStreamSynchronize(c->st));
		at += tot[i];
	}
	return (int64_t)n;
}

extern "C" void yakamd_hmopt_init(yakamd_hmopt_t *opt)
{
	memset(opt, 0, sizeof(yakamd_hmopt_t));
	opt->min_cnt = 1;
	opt->print_pairs = 0;
	opt->batch_keys = HM_BATCH_DEFAULT;
}

/* the command: per range the tallies, and with print_pairs the range's records copied back and written as K lines; G and P lines after the last
 * range.  The pairs of a range are counted before they are written, so one range's records are all the list memory there is */
extern "C" int yakamd_hetmers(const yakamd_hmopt_t *opt, const yak_ch_t *ch, const char *out_fn)
{
	yakamd_ctx *c = hm_ctx(ch, opt->min_cnt, "yakamd_hetmers");
	if (!c) return -1;
	HIPCK(hipSetDevice(c->dev));
	const int k = ch->k, min_cnt = opt->min_cnt;
	const hipStream_t st = c->st;
	const std::vector<Range> ranges = yk_ctx_ranges(c, 0, c->P, hm_batch(opt->batch_keys), false);
	GrowBuf d_list, d_tally;
	StagedRange s;
	PairScratch ps;
	const size_t tally_bytes = (size_t)NC * NC * 8 + 64;            /* J, then the five group counts */
	if (!d_tally.fit(tally_bytes)) return fail("yakamd_hetmers: no device memory for the histogram");
	HIPCK(hipMemsetAsync(d_tally.p, 0, tally_bytes, st));
	u64 *d_joint = (u64*)d_tally.p, *d_group = d_joint + (size_t)NC * NC;
	OutFile of;
	if (!of.open(out_fn)) return fail("yakamd_hetmers: cannot write '%s'", out_fn);
	FILE *out = of.f;
	fprintf(out, "#hetmers\tk=%d\tmin_cnt=%d\n", k, min_cnt);
	std::vector<yakamd_hetpair_t> recs;
	std::string text;
	u64 n_pairs = 0;
	for (const Range &r : ranges) {
		if (hm_stage(s, c, r)) return -1;
		if (yk_launch_hetmer(0, s.d_img, s.off(), r.n(), r.hi - r.lo, r.lo, min_cnt, img_view(c), d_joint, d_group, 0, 0, 0, st))
			return fail("yakamd_hetmers: the join did not launch");
		if (opt->print_pairs) {
			u64 tot = 0;
			if (ps.count(c, r, s, min_cnt, st, &tot)) return -1;
			if (tot) {
				if (!d_list.fit(tot * sizeof(yakamd_hetpair_t))) return fail("yakamd_hetmers: no device memory for %llu pairs", (unsigned long long)tot);
				if (ps.write(c, r, s, min_cnt, d_list.p, st)) return -1;
				HIPCK(hipStreamSynchronize(st));
				recs.resize(tot);
				if (yakamd_memcpy_d2h(recs.data(), d_list.p, tot * sizeof(yakamd_hetpair_t)) != 0) return -1;
				text.clear();
				char a[32], b[32], num[48];
				for (const yakamd_hetpair_t &p : recs) {
					kmer_text(a, p.x, k); kmer_text(b, p.y, k);
					text.append("K\t").append(a, k).append(num, (size_t)snprintf(num, sizeof num, "\t%u\t", p.cx)).append(b, k)
					    .append(num, (size_t)snprintf(num, sizeof num, "\t%u\n", p.cy));
				}
				if (fwrite(text.data(), 1, text.size(), out) != text.size()) return fail("yakamd_hetmers: cannot write '%s'", of.name);
				n_pairs += tot;
			}
		}
		HIPCK(hipStreamSynchronize(st));
	}
	std::vector<u64> tally(tally_bytes / 8);
	HIPCK(hipStreamSynchronize(st));
	if (yakamd_memcpy_d2h(tally.data(), d_tally.p, tally_bytes) != 0) return -1;
	const u64 *J = tally.data(), *G = J + (size_t)NC * NC;
	for (int s = 1; s <= 4; ++s) fprintf(out, "G\t%d\t%llu\n", s, (unsigned long long)G[s]);
	u64 sum = 0;
	for (int lo = 0; lo < NC; ++lo)
		for (int hi = 0; hi < NC; ++hi)
			if (J[(size_t)lo * NC + hi]) { sum += J[(size_t)lo * NC + hi]; fprintf(out, "P\t%d\t%d\t%llu\n", lo, hi, (unsigned long long)J[(size_t)lo * NC + hi]); }
	if (opt->print_pairs && sum != n_pairs) return fail("yakamd_hetmers: %llu pairs listed, %llu counted", (unsigned long long)n_pairs, (unsigned long long)sum);
	if (!of.finish()) return fail("yakamd_hetmers: cannot write '%s'", of.name);
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] hetmers: %zu ranges of keys, %llu pairs\n", ranges.size(), (unsigned long long)sum);
	return 0;
}
