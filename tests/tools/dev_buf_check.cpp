/* dev_buf_check.cpp -- the owner types of yak_amd/csrc/dev_buf.h over a pool made of malloc: every block is freed once, a DevVec frees before it
 * allocates and forgets its capacity when an allocation fails.  A program of its own (tests/test_dev_buf.py builds it with the address and
 * undefined-behaviour sanitizers: a block freed twice or used after its free stops it); prints `ok`. */
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>
#include <map>
#include <vector>
#include <algorithm>
#include "../../yak_amd/csrc/dev_buf.h"

/* ---- the pool: live blocks with their sizes, the high-water mark of live bytes, a switch that fails the next allocation ---- */
static std::map<void*, size_t> g_live;
static size_t g_bytes = 0, g_peak = 0;
static int g_double_free = 0, g_errors = 0;
static bool g_fail_next = false;

void *yk_pool_alloc(size_t bytes, bool)
{
	if (g_fail_next) { g_fail_next = false; return 0; }
	void *p = malloc(bytes);
	g_live[p] = bytes; g_bytes += bytes; g_peak = std::max(g_peak, g_bytes);
	return p;
}
void yk_pool_free(void *p)
{
	auto it = g_live.find(p);
	if (it == g_live.end()) { ++g_double_free; return; }         /* not live: freed before, or never handed out */
	g_bytes -= it->second; g_live.erase(it);
	free(p);
}
int yk_set_error(const char *, ...) { ++g_errors; return -1; }

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #x); ++g_bad; } } while (0)
static size_t live() { return g_live.size(); }

static void dev_buf()
{
	{
		DevBuf<int> a;
		CHECK(a.alloc(10) == 0 && a.get() && live() == 1);
		DevBuf<int> b(std::move(a));                              /* move-construct */
		CHECK(!a.get() && b.get() && live() == 1);
		DevBuf<int> c;
		CHECK(c.alloc(5) == 0 && live() == 2);
		c = std::move(b);                                         /* move-assign: c's own block goes */
		CHECK(!b.get() && c.get() && live() == 1);
		DevBuf<int> &same = c;
		c = std::move(same);                                      /* self-move-assign keeps the block */
		CHECK(c.get() && live() == 1);
		c.reset();
		CHECK(!c.get() && live() == 0);
		c.reset();                                                /* (twice is nothing) */
		CHECK(c.alloc(3) == 0 && live() == 1);
		int *raw = c.release();                                   /* handed out: the owner no longer frees it */
		CHECK(!c.get() && live() == 1);
		yk_pool_free(raw);
		CHECK(live() == 0);
		CHECK(c.alloc(7) == 0 && c.alloc(9) == 0 && live() == 1); /* alloc on a full owner frees first */
		DevBuf<int> d;
		CHECK(d.alloc(2) == 0 && live() == 2);
	}                                                             /* scope exit */
	CHECK(live() == 0 && g_double_free == 0);
	g_fail_next = true;
	DevBuf<int> f;
	CHECK(f.alloc(4) == -1 && !f.get() && g_errors == 1 && live() == 0);
}

static void dev_vec()
{
	DevVec<double> v;
	CHECK(v.get() == 0 && v.cap() == 0);
	CHECK(v.reserve(100) == 0 && v.cap() == 100 && live() == 1);
	double *p = v.get();
	CHECK(v.reserve(100) == 0 && v.reserve(1) == 0 && v.get() == p && v.cap() == 100);   /* n <= cap: the same buffer */
	g_peak = g_bytes;
	CHECK(v.reserve(250) == 0 && v.cap() == 250 && live() == 1);
	CHECK(g_peak == 250 * sizeof(double));                       /* max(old, new), not old + new: freed before allocated */
	g_peak = g_bytes;
	CHECK(v.reserve(251) == 0 && g_peak == 251 * sizeof(double));
	const int errors = g_errors;
	g_fail_next = true;
	CHECK(v.reserve(1000) == -1 && v.get() == 0 && v.cap() == 0 && live() == 0 && g_errors == errors + 1);
	CHECK(v.reserve(10) == 0 && v.get() != 0 && v.cap() == 10 && live() == 1);   /* a smaller n allocates: no stale capacity */
	DevVec<double> w(std::move(v));
	CHECK(v.get() == 0 && v.cap() == 0 && w.cap() == 10 && live() == 1);
	v = std::move(w);
	CHECK(w.get() == 0 && w.cap() == 0 && v.cap() == 10 && live() == 1);
	v.reset();
	CHECK(v.get() == 0 && v.cap() == 0 && live() == 0 && g_double_free == 0);
}

/* an owner and a view of it, as the engine's kept batches are: the view follows the records, whoever owns them */
struct KeptLike { DevBuf<long> own; long *view = 0; std::vector<int> host; };

static void owner_and_view_in_a_vector()
{
	std::vector<KeptLike> v;
	long borrowed[4];
	for (int i = 0; i < 100; ++i) {                               /* (the vector reallocates several times on the way) */
		KeptLike k;
		if (i % 3) { CHECK(k.own.alloc(8) == 0); k.view = k.own.get(); }
		else k.view = borrowed;
		k.host.assign(5, i);
		v.push_back(std::move(k));
	}
	CHECK(live() == 66);
	for (auto &k : v) CHECK(k.view == (k.own ? k.own.get() : borrowed));
	std::vector<DevBuf<long>> taken;
	for (size_t i = 0; i < v.size(); i += 2) taken.push_back(std::move(v[i].own));   /* half of them moved out */
	CHECK(live() == 66);
	v.clear();
	CHECK(live() == 33);
	taken.clear();
	CHECK(live() == 0 && g_double_free == 0);
}

int main()
{
	dev_buf();
	dev_vec();
	owner_and_view_in_a_vector();
	CHECK(live() == 0 && g_bytes == 0 && g_double_free == 0);
	if (g_bad) return 1;
	printf("ok\n");
	return 0;
}
