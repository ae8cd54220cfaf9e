/* rec_fmt_check.cpp -- the record formats of yak_amd/csrc/yk_device.h (RecFmt) on the host: the predicate "tagged records fit" against the tagged
 * record's definition written out for every k and prefix, the bytes of the four formats and how many Rec elements hold n records of each, and the
 * layout of Chunk2 the level-2 kernels read (its size and the offset of `fmt`, the field that was `pad`).  A program of its own
 * (tests/test_rec_fmt.py builds it with the address and undefined-behaviour sanitizers, the HIP headers on the include path); prints `ok`. */
#include <stdio.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../yak_amd/csrc/yk_device.h"

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { if (g_bad < 20) fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #x); ++g_bad; } } while (0)

static int64_t g_rec8 = -1;                                      /* >= 0: what YAKAMD_REC8 is set to */
extern "C" int64_t yk_knob(const char *name, int64_t dflt) { return g_rec8 >= 0 && !strcmp(name, "YAKAMD_REC8") ? g_rec8 : dflt; }

/* The definition: a tagged record is (hash >> pre) << 12 | 12 tag bits in one 64-bit word, so the hash above `pre` must come back whole from above
 * the tag.  The hash of a k-mer of k < 32 bases has 2k bits; the kernels that write the format (k_xpart<3>, k_xpart_wcs<true>) take those k only,
 * and no more than 2^10 buckets */
static bool fits_by_definition(int k, int pre)
{
	if (k >= 32 || pre > 10) return false;
	const uint64_t largest = (1ull << (2 * k)) - 1, above = pre < 64 ? largest >> pre : 0;
	return (above << YK_R8_TAG_BITS) >> YK_R8_TAG_BITS == above;
}

int main()
{
	for (int k = 1; k <= 63; ++k)
		for (int pre = 0; pre <= 16; ++pre) {
			const bool want = fits_by_definition(k, pre);
			if (yk_tagged_fits(k, pre) != want) { if (g_bad < 20) fprintf(stderr, "k %d, pre %d: yk_tagged_fits says %d, the definition %d\n", k, pre, !want, want); ++g_bad; }
			g_rec8 = 0;
			CHECK(!yk_tagged_fits(k, pre));                         /* the switch turns the format off everywhere */
			g_rec8 = -1;
		}
	CHECK(YK_R8_TAG_BITS == 12 && YK_R8_TOGGLE == 1u << 10);

	CHECK(sizeof(Rec) == 16);
	CHECK(yk_rec_bytes(YK_FMT_POS) == 16 && yk_rec_bytes(YK_FMT_TAGGED) == 8 && yk_rec_bytes(YK_FMT_HASH) == 8 && yk_rec_bytes(YK_FMT_HASH_RNG) == 8);
	for (size_t n = 0; n < 9; ++n) {
		CHECK(yk_rec_units(YK_FMT_POS, n) == n);
		CHECK(yk_rec_units(YK_FMT_TAGGED, n) == (n + 1) / 2 && yk_rec_units(YK_FMT_HASH, n) == (n + 1) / 2 && yk_rec_units(YK_FMT_HASH_RNG, n) == (n + 1) / 2);
	}
	CHECK(yk_rec_units(YK_FMT_TAGGED, ((size_t)1 << 34) + 1) == ((size_t)1 << 33) + 1);   /* beyond 2^32 records: a rank of a multi-GPU job */

	/* what the device compares Chunk2::fmt with (kern_count.inc p2_load: 1 = tagged), and where it reads it */
	CHECK(YK_FMT_POS == 0 && YK_FMT_TAGGED == 1);
	CHECK(sizeof(Chunk2) == 40 && offsetof(Chunk2, fmt) == 28);
	CHECK(sizeof(((Chunk2*)0)->fmt) == 4);

	if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
	printf("ok\n");
	return 0;
}
