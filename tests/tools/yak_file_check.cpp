/* yak_file_check.cpp -- the .yak reader of yak_amd/csrc/yak_file.h against the three parsers it replaced, restated here as they stood: read_yak
 * (restore; yak_api.cpp), parse_yak_image (the unsharded copy; yak_api.cpp), and read_head with BodyReader (inspect; yak_inspect.cpp).  Their
 * messages became return codes, read_yak takes the open stream instead of the name; nothing else changed.  Inputs: the golden tables named in
 * argv, a few hundred random small images, one image cut at every byte offset, and headers that each caller refuses.  A program of its own
 * (tests/test_yak_file.py builds it with the address and undefined-behaviour sanitizers); prints `ok`. */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <string>
#include "../../yak_amd/csrc/yak_file.h"

static int g_bad = 0;
static std::string g_case;
#define CHECK(x) do { if (!(x)) { if (g_bad < 20) fprintf(stderr, "%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #x, g_case.c_str()); ++g_bad; } } while (0)

typedef std::vector<uint8_t> Image;

/* ---- the old parsers ---- */
enum OldRc { OLD_OK = 0, OLD_FAIL, OLD_MAGIC, OLD_BITS, OLD_CORRUPT, OLD_RANGE, OLD_TRUNC_HEAD, OLD_TRUNC_BODY };

/* yak_api.cpp, read_yak(fn, ...) after its fopen */
static OldRc old_read_yak(FILE *fp, uint32_t hdr[3], std::vector<uint32_t> &caps, std::vector<uint32_t> &sizes, std::vector<uint64_t> &keys)
{
	char magic[4];
	if (fread(magic, 1, 4, fp) != 4) return OLD_FAIL;
	if (strncmp(magic, YAK_MAGIC, 4) != 0) return OLD_MAGIC;
	if (fread(hdr, 4, 3, fp) != 3) return OLD_FAIL;
	if (hdr[2] != YAK_COUNTER_BITS) return OLD_BITS;
	if (hdr[1] < YAK_COUNTER_BITS || hdr[1] > 24) return OLD_FAIL;
	const int P = 1 << hdr[1];
	caps.assign(P, 0); sizes.assign(P, 0); keys.clear();
	for (int p = 0; p < P; ++p) {
		uint32_t u[2];
		if (fread(u, 4, 2, fp) != 2) break;
		if (u[0] > (1u << 31) || (u[0] & (u[0] - 1)) != 0 || u[1] > u[0]) return OLD_CORRUPT;
		caps[p] = u[0]; sizes[p] = u[1];
		const size_t at = keys.size();
		keys.resize(at + u[1]);
		if (u[1] && fread(&keys[at], 8, u[1], fp) != u[1]) break;
	}
	return OLD_OK;
}

/* yak_api.cpp, parse_yak_image */
static bool old_parse_yak_image(const uint8_t *img, size_t sz, uint32_t hdr[3], std::vector<uint32_t> &caps, std::vector<uint32_t> &sizes, std::vector<uint64_t> &keys)
{
	if (sz < 16 || memcmp(img, YAK_MAGIC, 4) != 0) return false;
	memcpy(hdr, img + 4, 12);
	const int P = 1 << hdr[1];
	caps.assign(P, 0); sizes.assign(P, 0); keys.clear();
	size_t off = 16;
	for (int p = 0; p < P; ++p) {
		if (off + 8 > sz) return false;
		uint32_t u[2]; memcpy(u, img + off, 8); off += 8;
		if (off + (size_t)8 * u[1] > sz) return false;
		caps[p] = u[0]; sizes[p] = u[1];
		const size_t at = keys.size();
		keys.resize(at + u[1]);
		if (u[1]) memcpy(&keys[at], img + off, (size_t)8 * u[1]);
		off += (size_t)8 * u[1];
	}
	return true;
}

/* yak_inspect.cpp, read_head */
struct OldHead { int k, pre; };
static OldRc old_read_head(FILE *fp, OldHead *h)
{
	char magic[4];
	uint32_t t[3];
	if (fread(magic, 1, 4, fp) != 4 || fread(t, 4, 3, fp) != 3) return OLD_TRUNC_HEAD;
	if (memcmp(magic, YAK_MAGIC, 4) != 0) return OLD_MAGIC;
	if (t[2] != YAK_COUNTER_BITS) return OLD_BITS;
	if (t[0] < 1 || t[0] > 63 || t[1] < YAK_COUNTER_BITS || t[1] > 30) return OLD_RANGE;
	h->k = (int)t[0]; h->pre = (int)t[1];
	return OLD_OK;
}

/* yak_inspect.cpp, Batch and BodyReader */
struct OldBatch {
	std::vector<uint64_t> keys, off;
	int lo = 0;
	void clear() { keys.clear(); off.clear(); }
	int n_sub() const { return (int)off.size() - 1; }
};
struct OldBodyReader {
	FILE *fp = 0;
	int P = 0, cur = 0;
	uint64_t rest = 0;
	bool in_sub = false;
	bool bad = false;
	bool done() const { return cur >= P; }
	bool next(int64_t cap, OldBatch *b)
	{
		b->clear();
		b->lo = cur;
		b->off.push_back(0);
		while (cur < P) {
			if (!in_sub) {
				uint32_t t[2];
				if (fread(t, 4, 2, fp) != 2) return fail();
				rest = t[1]; in_sub = true;
			}
			const uint64_t room = (uint64_t)cap - b->keys.size(), take = rest < room ? rest : room;
			if (take) {
				const size_t at = b->keys.size();
				b->keys.resize(at + take);
				if (fread(b->keys.data() + at, 8, take, fp) != take) return fail();
				rest -= take;
			}
			b->off.push_back(b->keys.size());
			if (rest) break;
			in_sub = false; ++cur;
			if ((int64_t)b->keys.size() >= cap) break;
		}
		return true;
	}
	bool fail() { bad = true; return false; }      /* (the message named `cur`) */
};

/* ---- what each caller makes of a header: yak_file.cpp read_table_file, yak_inspect.cpp read_head ---- */
static OldRc restore_view(YakStatus st, const YakHeader &h)
{
	if (st == YAK_BAD_MAGIC) return OLD_MAGIC;
	if (st == YAK_BAD_BITS) return OLD_BITS;
	return st == YAK_OK && h.pre >= YAK_COUNTER_BITS && h.pre <= 24 ? OLD_OK : OLD_FAIL;
}
static OldRc inspect_view(YakStatus st, const YakHeader &h)
{
	if (st == YAK_SHORT_HEADER) return OLD_TRUNC_HEAD;
	if (st == YAK_BAD_MAGIC) return OLD_MAGIC;
	if (st == YAK_BAD_BITS) return OLD_BITS;
	return h.k < 1 || h.k > 63 || h.pre < YAK_COUNTER_BITS || h.pre > 30 ? OLD_RANGE : OLD_OK;
}

/* ---- sources ---- */
static FILE *open_image(const Image &img, size_t n)                  /* the first n bytes as a stream (n > 0) */
{
	FILE *fp = fmemopen((void*)img.data(), n, "rb");
	if (!fp) { perror("fmemopen"); exit(2); }
	return fp;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static void put32(Image &img, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); img.insert(img.end(), b, b + 4); }
static void put64(Image &img, uint64_t v) { uint8_t b[8]; memcpy(b, &v, 8); img.insert(img.end(), b, b + 8); }
static Image header_image(const char *magic, uint32_t k, uint32_t pre, uint32_t bits)
{
	Image img(magic, magic + 4);
	put32(img, k); put32(img, pre); put32(img, bits);
	return img;
}

/* a well-formed image with pre = 10: about one sub-table in `one_in` holds keys, 0 to 40 of them, under a capacity that is a power of two (an empty
 * one: 0 or a power of two), and one sub-table is filled to its capacity */
static Image random_image(int one_in)
{
	const int P = 1 << 10, full = (int)(rnd() % P);
	Image img = header_image(YAK_MAGIC, 1 + (uint32_t)(rnd() % 63), 10, YAK_COUNTER_BITS);
	for (int p = 0; p < P; ++p) {
		uint32_t size = rnd() % (uint64_t)one_in == 0 ? (uint32_t)(rnd() % 41) : 0, cap = 0;
		if (p == full) { cap = 1u << (rnd() % 6); size = cap; }
		else if (size || rnd() % 2) { cap = 1; while (cap < size) cap <<= 1; cap <<= rnd() % 3; }
		put32(img, cap); put32(img, size);
		for (uint32_t j = 0; j < size; ++j) put64(img, rnd());
	}
	return img;
}

/* ---- a well-formed image: everything the new reader gives equals what the old parsers gave ---- */
static void well_formed(const Image &img)
{
	uint32_t hdr[3], hdr2[3];
	std::vector<uint32_t> caps0, sizes0, caps1, sizes1;
	std::vector<uint64_t> keys0, keys1;
	FILE *fp = open_image(img, img.size());
	const OldRc rc = old_read_yak(fp, hdr, caps0, sizes0, keys0);
	fclose(fp);
	CHECK(rc == OLD_OK);
	CHECK(old_parse_yak_image(img.data(), img.size(), hdr2, caps1, sizes1, keys1));
	CHECK(memcmp(hdr, hdr2, 12) == 0 && caps0 == caps1 && sizes0 == sizes1 && keys0 == keys1);
	if (rc != OLD_OK) return;
	const int pre = (int)hdr[1], P = 1 << pre;

	/* the whole table, from the stream and from memory */
	for (int from_file = 0; from_file < 2; ++from_file) {
		FILE *f = from_file ? open_image(img, img.size()) : 0;
		YakSrc src = from_file ? YakSrc::file(f) : YakSrc::memory(img.data(), img.size());
		YakHeader h;
		std::vector<uint32_t> caps, sizes;
		std::vector<uint64_t> keys;
		YakBody where;
		CHECK(yak_read_header(src, &h) == YAK_OK && h.k == hdr[0] && h.pre == hdr[1] && h.bits == hdr[2]);
		CHECK(restore_view(YAK_OK, h) == OLD_OK);
		CHECK(yak_read_all(src, pre, caps, sizes, keys, &where) == YAK_OK && where.done());
		CHECK(caps == caps0 && sizes == sizes0 && keys == keys0);
		if (f) fclose(f);
	}

	/* the batches */
	uint64_t first = 0;
	for (int p = 0; p < P && !first; ++p) first = sizes0[p];
	const int64_t total = (int64_t)keys0.size();
	const int64_t budgets[] = { 1, 2, 7, (int64_t)first, (int64_t)first - 1, (int64_t)first + 1, total, total + 5, INT64_MAX };
	for (int64_t cap : budgets) {
		if (cap < 1) continue;
		FILE *f_old = open_image(img, img.size()), *f_new = open_image(img, img.size());
		OldHead oh;
		CHECK(old_read_head(f_old, &oh) == OLD_OK);
		OldBodyReader rd;
		rd.fp = f_old; rd.P = 1 << oh.pre;
		YakSrc s_file = YakSrc::file(f_new), s_mem = YakSrc::memory(img.data(), img.size());
		YakHeader h;
		CHECK(yak_read_header(s_file, &h) == YAK_OK && yak_read_header(s_mem, &h) == YAK_OK && inspect_view(YAK_OK, h) == OLD_OK && (int)h.pre == oh.pre);
		YakBody b_file(&s_file, (int)h.pre), b_mem(&s_mem, (int)h.pre);
		std::vector<uint64_t> all;
		OldBatch ob;
		YakBatch nb, mb;
		int guard = 0;
		while (!rd.done() && ++guard < (1 << 22)) {
			CHECK(!b_file.done() && !b_mem.done());
			const bool ok = rd.next(cap, &ob);
			CHECK(ok && b_file.next(cap, &nb) == YAK_OK && b_mem.next(cap, &mb) == YAK_OK);
			if (!ok) break;
			CHECK(nb.lo == ob.lo && nb.off == ob.off && nb.keys == ob.keys && b_file.cur == rd.cur);   /* lo, off[] and the split rule */
			CHECK(mb.lo == ob.lo && mb.off == ob.off && mb.keys == ob.keys && b_mem.cur == rd.cur);
			CHECK(nb.cap.size() == (size_t)nb.n_sub() && nb.cap == mb.cap);
			for (int j = 0; j < nb.n_sub() && (size_t)j < nb.cap.size(); ++j) CHECK(nb.cap[j] == caps0[nb.lo + j]);
			CHECK((int64_t)nb.keys.size() <= cap);
			all.insert(all.end(), nb.keys.begin(), nb.keys.end());
		}
		CHECK(b_file.done() && b_mem.done());
		CHECK(all == keys0);                                          /* the batches, concatenated, are yak_read_all's keys */
		fclose(f_old); fclose(f_new);
	}
}

/* ---- one image cut at every byte offset ---- */
static void cut_everywhere(const Image &img)
{
	const int P = 1 << 10;
	std::vector<size_t> end(P);                                       /* the offset behind sub-table p */
	size_t off = 16;
	for (int p = 0; p < P; ++p) { uint32_t u[2]; memcpy(u, img.data() + off, 8); off += 8 + (size_t)8 * u[1]; end[p] = off; }
	CHECK(off == img.size());
	for (size_t c = 0; c < img.size(); ++c) {
		g_case = "cut at " + std::to_string(c);
		int want = 0;
		while (want < P && end[want] <= c) ++want;                    /* the first sub-table that is not whole */
		for (int from_file = 0; from_file < 2; ++from_file) {
			if (from_file && c == 0) continue;                        /* (no stream of no bytes) */
			FILE *f = from_file ? open_image(img, c) : 0;
			YakSrc src = from_file ? YakSrc::file(f) : YakSrc::memory(img.data(), c);
			YakHeader h;
			const YakStatus st = yak_read_header(src, &h);
			CHECK(st == (c < 16 ? YAK_SHORT_HEADER : YAK_OK));
			if (c < 16 && f) { OldHead oh; rewind(f); CHECK(old_read_head(f, &oh) == OLD_TRUNC_HEAD && inspect_view(st, h) == OLD_TRUNC_HEAD); }
			if (st == YAK_OK) {
				std::vector<uint32_t> caps, sizes;
				std::vector<uint64_t> keys;
				YakBody where;
				CHECK(yak_read_all(src, (int)h.pre, caps, sizes, keys, &where) == YAK_TRUNCATED && where.cur == want);
			}
			if (f) fclose(f);
		}
		if (c < 16) continue;
		/* the old reader of inspect names the same sub-table, and so do the new batches: small batches at the odd offsets, inspect's own at the even ones */
		for (int64_t cap : { c & 1 ? (int64_t)7 : (int64_t)1 << 24 }) {
			FILE *f_old = open_image(img, c), *f_new = open_image(img, c);
			OldHead oh;
			YakHeader h;
			YakSrc src = YakSrc::file(f_new);
			CHECK(old_read_head(f_old, &oh) == OLD_OK && yak_read_header(src, &h) == YAK_OK);
			OldBodyReader rd;
			rd.fp = f_old; rd.P = 1 << oh.pre;
			YakBody body(&src, (int)h.pre);
			OldBatch ob;
			YakBatch nb;
			bool ok = true;
			YakStatus st = YAK_OK;
			while (ok && !rd.done()) { ok = rd.next(cap, &ob); st = body.next(cap, &nb); CHECK(ok == (st == YAK_OK)); }
			CHECK(!ok && rd.bad && rd.cur == want && st == YAK_TRUNCATED && body.cur == want);
			fclose(f_old); fclose(f_new);
		}
	}
}

/* ---- headers and sub-table headers that a caller refuses ---- */
static void one_header(const char *magic, uint32_t k, uint32_t pre, uint32_t bits, YakStatus want)
{
	Image img = header_image(magic, k, pre, bits);
	put32(img, 0); put32(img, 0);                                     /* (a body too short for any pre: no old parser gets further than its checks) */
	g_case = "header k " + std::to_string(k) + " pre " + std::to_string(pre) + " bits " + std::to_string(bits);
	YakSrc src = YakSrc::memory(img.data(), img.size());
	YakHeader h = { 0, 0, 0 };
	const YakStatus st = yak_read_header(src, &h);
	CHECK(st == want);
	/* restore: its limits, against read_yak (which fails on the short body only after the checks: OLD_OK here means the header passed) */
	uint32_t hdr[3];
	std::vector<uint32_t> caps, sizes;
	std::vector<uint64_t> keys;
	FILE *fp = open_image(img, img.size());
	const OldRc rc = old_read_yak(fp, hdr, caps, sizes, keys);
	fclose(fp);
	CHECK(restore_view(st, h) == rc);
	/* inspect: its limits, against read_head */
	fp = open_image(img, img.size());
	OldHead oh;
	CHECK(inspect_view(st, h) == old_read_head(fp, &oh));
	fclose(fp);
}

static void bad_subtable(uint32_t cap, uint32_t size)
{
	g_case = "sub-table header " + std::to_string(cap) + " / " + std::to_string(size);
	Image img = header_image(YAK_MAGIC, 31, 10, YAK_COUNTER_BITS);
	const int at = (int)(rnd() % 1024);
	for (int p = 0; p < at; ++p) { put32(img, 0); put32(img, 0); }
	put32(img, cap); put32(img, size);
	for (int j = 0; j < 4; ++j) put64(img, rnd());                    /* (never read) */
	uint32_t hdr[3];
	std::vector<uint32_t> caps, sizes;
	std::vector<uint64_t> keys;
	FILE *fp = open_image(img, img.size());
	CHECK(old_read_yak(fp, hdr, caps, sizes, keys) == OLD_CORRUPT);
	fclose(fp);
	for (int from_file = 0; from_file < 2; ++from_file) {
		FILE *f = from_file ? open_image(img, img.size()) : 0;
		YakSrc src = from_file ? YakSrc::file(f) : YakSrc::memory(img.data(), img.size());
		YakHeader h;
		YakBody where;
		CHECK(yak_read_header(src, &h) == YAK_OK);
		CHECK(yak_read_all(src, (int)h.pre, caps, sizes, keys, &where) == YAK_BAD_SUBTABLE && where.cur == at && where.cap == cap && where.size == size);
		if (f) fclose(f);
	}
}

static bool read_file(const char *fn, Image *img)
{
	FILE *fp = fopen(fn, "rb");
	if (!fp) return false;
	uint8_t buf[65536];
	size_t n;
	img->clear();
	while ((n = fread(buf, 1, sizeof buf, fp)) > 0) img->insert(img->end(), buf, buf + n);
	fclose(fp);
	return true;
}

int main(int argc, char **argv)
{
	/* the golden tables: through fopen() too, as restore and inspect open them */
	for (int i = 1; i < argc; ++i) {
		g_case = argv[i];
		Image img;
		if (!read_file(argv[i], &img)) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
		well_formed(img);
		FILE *fp = fopen(argv[i], "rb");
		YakSrc src = YakSrc::file(fp), mem = YakSrc::memory(img.data(), img.size());
		YakHeader h, hm;
		std::vector<uint32_t> caps, sizes, caps_m, sizes_m;
		std::vector<uint64_t> keys, keys_m;
		CHECK(yak_read_header(src, &h) == YAK_OK && yak_read_header(mem, &hm) == YAK_OK && h.k == hm.k && h.pre == hm.pre);
		CHECK(yak_read_all(src, (int)h.pre, caps, sizes, keys) == YAK_OK && yak_read_all(mem, (int)hm.pre, caps_m, sizes_m, keys_m) == YAK_OK);
		CHECK(caps == caps_m && sizes == sizes_m && keys == keys_m && fgetc(fp) == EOF);
		fclose(fp);
	}
	/* random small images */
	for (int i = 0; i < 300; ++i) {
		g_case = "random image " + std::to_string(i);
		well_formed(random_image(i % 3 == 0 ? 8 : 40));
	}
	{	/* all sub-tables empty but the full one */
		g_case = "nearly empty image";
		well_formed(random_image(1 << 30));
	}
	/* one image of about 9 KB, cut at every byte offset */
	Image img;
	do img = random_image(150); while (img.size() < 8800 || img.size() > 9600);
	cut_everywhere(img);
	/* bad headers */
	one_header("YAK\1", 31, 10, YAK_COUNTER_BITS, YAK_BAD_MAGIC);
	one_header("KAY\2", 31, 10, YAK_COUNTER_BITS, YAK_BAD_MAGIC);
	one_header(YAK_MAGIC, 31, 10, 8, YAK_BAD_BITS);
	one_header(YAK_MAGIC, 31, 10, 12, YAK_BAD_BITS);
	for (uint32_t pre : { 9u, 10u, 24u, 25u, 30u, 31u }) one_header(YAK_MAGIC, 31, pre, YAK_COUNTER_BITS, YAK_OK);
	for (uint32_t k : { 0u, 1u, 63u, 64u }) one_header(YAK_MAGIC, k, 10, YAK_COUNTER_BITS, YAK_OK);
	bad_subtable(3, 1);                                                /* no power of two */
	bad_subtable(48, 40);
	bad_subtable(0x80000001u, 5);                                      /* above 2^31 */
	bad_subtable(0xffffffffu, 0xffffffffu);
	bad_subtable(8, 9);                                                /* more keys than slots */
	bad_subtable(0, 1);
	if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
	printf("ok\n");
	return 0;
}
