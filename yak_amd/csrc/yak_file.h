/* yak_file.h -- the one reader of the .yak table format (reference htab.c:373-394, DESIGN.md "The .yak format in one place"): the 16-byte header --
 * the magic, then k, pre and the counter bits as 32-bit words --, then for each of the 1 << pre sub-tables its capacity and its size as 32-bit
 * words and `size` stored keys of 64 bits in ascending slot order.  Restore, the unsharded copy of a table, inspect and yakamd_yak_header() read
 * through it, from a file or from an image in memory.  It returns statuses and words no message: the callers keep their own texts, and their own
 * limits for k and pre.  A body that ends early is an error here, for every caller.
 * Host C++ alone: tests/tools/yak_file_check.cpp holds it against the three parsers it replaced. */
#ifndef YK_YAK_FILE_H
#define YK_YAK_FILE_H
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/yak.h"

/* where the bytes come from: an open FILE*, or `size` bytes at `mem` */
struct YakSrc {
	FILE *fp = 0;
	const uint8_t *mem = 0;
	size_t size = 0, at = 0;
	static YakSrc file(FILE *fp) { YakSrc s; s.fp = fp; return s; }
	static YakSrc memory(const void *p, size_t n) { YakSrc s; s.mem = (const uint8_t*)p; s.size = n; return s; }
	/* the next n bytes, all of them or false */
	bool read(void *dst, size_t n)
	{
		if (fp) return n == 0 || fread(dst, 1, n, fp) == n;
		if (n > size - at) return false;
		if (n) memcpy(dst, mem + at, n);
		at += n;
		return true;
	}
};

enum YakStatus { YAK_OK = 0, YAK_SHORT_HEADER, YAK_BAD_MAGIC, YAK_BAD_BITS, YAK_TRUNCATED, YAK_BAD_SUBTABLE };

struct YakHeader { uint32_t k, pre, bits; };

/* the header.  YAK_BAD_BITS leaves *h filled (the caller's message names the saved bits).  The ranges of k and pre are the caller's to check */
static inline YakStatus yak_read_header(YakSrc &src, YakHeader *h)
{
	uint8_t b[16];
	if (!src.read(b, 16)) return YAK_SHORT_HEADER;
	if (memcmp(b, YAK_MAGIC, 4) != 0) return YAK_BAD_MAGIC;
	uint32_t t[3];
	memcpy(t, b + 4, 12);
	h->k = t[0]; h->pre = t[1]; h->bits = t[2];
	return t[2] == YAK_COUNTER_BITS ? YAK_OK : YAK_BAD_BITS;
}

/* one batch of the body: the keys of sub-tables [lo, lo + off.size() - 1) in file order, off[j] = keys before sub-table lo + j, cap[j] its saved
 * capacity.  A sub-table larger than the room left is split: the batch ends with its first part and the next one starts with the rest, under the
 * same index */
struct YakBatch {
	std::vector<uint64_t> keys, off;
	std::vector<uint32_t> cap;
	int lo = 0;
	void clear() { keys.clear(); off.clear(); cap.clear(); }
	int n_sub() const { return (int)off.size() - 1; }
};

/* the body behind the header, read sub-table by sub-table (inspect.c:47-62) */
struct YakBody {
	YakSrc *src = 0;
	int P = 0, cur = 0;                  /* sub-tables; the next one: the one a status other than YAK_OK names */
	uint64_t rest = 0;                   /* keys of sub-table cur still to read */
	uint32_t cap = 0, size = 0;          /* its header */
	bool in_sub = false;                 /* which was read */
	bool strict = false;                 /* refuse a header that no table writes (yak_read_all) */
	YakBody() {}
	YakBody(YakSrc *s, int pre, bool strict_ = false) : src(s), P(1 << pre), strict(strict_) {}
	bool done() const { return cur >= P; }
	/* the next batch of about `cap_keys` keys; YAK_TRUNCATED on a short read, strict: YAK_BAD_SUBTABLE before the keys of such a header are read */
	YakStatus next(int64_t cap_keys, YakBatch *b)
	{
		b->clear();
		b->lo = cur;
		b->off.push_back(0);
		while (cur < P) {
			if (!in_sub) {
				uint32_t t[2];
				if (!src->read(t, 8)) return YAK_TRUNCATED;
				cap = t[0]; size = t[1];
				/* a capacity is 0 or a power of two <= 2^31 (khashl.h:155-158), and it holds its keys at <= 75 % load after the
				 * resize-before-put rule: anything else is a corrupt file */
				if (strict && (cap > (1u << 31) || (cap & (cap - 1)) != 0 || size > cap)) return YAK_BAD_SUBTABLE;
				rest = size; in_sub = true;
			}
			const uint64_t room = (uint64_t)cap_keys - b->keys.size(), take = rest < room ? rest : room;
			if (take) {
				const size_t at = b->keys.size();
				b->keys.resize(at + take);
				if (!src->read(b->keys.data() + at, (size_t)take * 8)) return YAK_TRUNCATED;
				rest -= take;
			}
			b->off.push_back(b->keys.size());
			b->cap.push_back(cap);
			if (rest) break;                                      /* split: the rest of sub-table cur opens the next batch */
			in_sub = false; ++cur;
			if ((int64_t)b->keys.size() >= cap_keys) break;
		}
		return YAK_OK;
	}
};

/* the whole body behind a header of `pre`: per sub-table its capacity and size, and all keys in file order.  Other than YAK_OK -- a short body, or
 * a sub-table header that no table writes -- with where->cur, where->cap and where->size telling which; the vectors are then no table */
static inline YakStatus yak_read_all(YakSrc &src, int pre, std::vector<uint32_t> &caps, std::vector<uint32_t> &sizes, std::vector<uint64_t> &keys, YakBody *where = 0)
{
	YakBody body(&src, pre, true);
	YakBatch b;
	YakStatus st = YAK_OK;
	caps.assign(body.P, 0); sizes.assign(body.P, 0); keys.clear();
	while (!body.done() && (st = body.next(INT64_MAX, &b)) == YAK_OK) {   /* (everything that is left, as one batch) */
		for (int j = 0; j < b.n_sub(); ++j) { caps[b.lo + j] = b.cap[j]; sizes[b.lo + j] += (uint32_t)(b.off[j + 1] - b.off[j]); }
		if (keys.empty()) keys.swap(b.keys);
		else keys.insert(keys.end(), b.keys.begin(), b.keys.end());
	}
	if (where) *where = body;
	return st;
}
#endif
