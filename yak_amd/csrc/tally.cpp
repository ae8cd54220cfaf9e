/* tally.cpp -- the counters behind tally.h: a fixed table of names and relaxed atomics, filled while the library is loaded */
#include "tally.h"
#include "yak_amd.h"
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {
enum { TALLY_MAX = 512, NAME_MAX_ = 96 };
struct Tally {
	char name[TALLY_MAX][NAME_MAX_];
	const char *names[TALLY_MAX];
	std::atomic<uint64_t> n[TALLY_MAX];
	int count;
	Tally() : count(0)
	{
		static const char *const ev[YKE_N] = {
			"event:rank_refused", "event:r2_used", "event:r2_refused", "event:par_ok", "event:par_fail", "event:lc2_passed_on", "event:ovf_groups",
			"event:ovf_more_groups", "event:slices", "event:early_slices", "event:fast_abandoned", "event:rng_sweeps", "event:own_sweeps",
			"event:pass2_none", "event:pass2_fused", "event:pass2_recount", "event:pass2_prefix" };
		for (int i = 0; i < TALLY_MAX; ++i) { n[i].store(0, std::memory_order_relaxed); names[i] = name[i]; name[i][0] = 0; }
		for (int i = 0; i < YKE_N; ++i) add(ev[i]);
	}
	int add(const char *s)
	{
		if (count >= TALLY_MAX || strlen(s) >= NAME_MAX_) { fprintf(stderr, "[yak_amd] tally: no room for %s\n", s); abort(); }
		strcpy(name[count], s);
		return count++;
	}
};
Tally &tally() { static Tally t; return t; }        /* built on first use: the registrations of other translation units may come first */
}

int yk_tally_register(const char *name)
{
	char buf[NAME_MAX_];
	size_t a = 0, b = strlen(name), o = 0;
	while (a < b && (name[a] == ' ' || name[a] == '\t')) ++a;
	while (b > a && (name[b - 1] == ' ' || name[b - 1] == '\t')) --b;
	if (b - a >= 2 && name[a] == '(' && name[b - 1] == ')') { ++a; --b; }
	for (size_t i = a; i < b && o + 1 < sizeof(buf); ++i) if (name[i] != ' ' && name[i] != '\t') buf[o++] = name[i];
	buf[o] = 0;
	Tally &t = tally();
	for (int i = 0; i < t.count; ++i) if (strcmp(t.name[i], buf) == 0) return i;
	return t.add(buf);
}

void yk_tally_bump(int id, uint64_t by) { tally().n[id].fetch_add(by, std::memory_order_relaxed); }

extern "C" int yakamd_tally_names(const char *const **names)
{
	Tally &t = tally();
	if (names) *names = t.names;
	return t.count;
}
extern "C" void yakamd_tally_read(uint64_t *out, int n)
{
	Tally &t = tally();
	for (int i = 0; i < n; ++i) out[i] = i < t.count ? t.n[i].load(std::memory_order_relaxed) : 0;
}
extern "C" void yakamd_tally_reset(void)
{
	Tally &t = tally();
	for (int i = 0; i < t.count; ++i) t.n[i].store(0, std::memory_order_relaxed);
}
