/* hpc_host.h -- homopolymer compression of a base image in plain C++: the host restatement of kern_hpc.inc, for
 * yakamd_hpc_host() and for the host code that must know where a compressed stream may be cut (yak_multi.cpp).  No device, no library state. */
#ifndef YK_HPC_HOST_H
#define YK_HPC_HOST_H
#include <stdint.h>

/* `out` receives the kept positions of a[0 .. n) -- 'A' 'C' 'G' 'T' for a valid one (nt4[byte] < 4), '\n' for any other -- and '\n' up to the next
 * multiple of 16; a position is dropped iff it and the one before it are valid and hold the same code.  Returns the number kept; out has room for
 * n rounded up to 16 and does not overlap a */
static inline int64_t yk_hpc_host(const unsigned char *nt4, const uint8_t *a, int64_t n, uint8_t *out)
{
	int64_t m = 0;
	unsigned prev = 4;                                         /* the code before: 4 = none or invalid */
	for (int64_t i = 0; i < n; ++i) {
		const unsigned c = nt4[a[i]];
		if (c < 4 && c == prev) continue;
		out[m++] = c < 4 ? (uint8_t)"ACGT"[c] : (uint8_t)'\n';
		prev = c < 4 ? c : 4;
	}
	for (int64_t i = m; i < ((m + 15) & ~(int64_t)15); ++i) out[i] = '\n';
	return m;
}

/* where a chunk that continues a[0 .. m) must begin so that its compressed form starts with exactly the last `want` kept positions of a[0 .. m):
 * the want-th kept position from the end (a run's first position).  -1 when a[0 .. m) holds fewer */
static inline int64_t yk_hpc_back(const unsigned char *nt4, const uint8_t *a, int64_t m, int64_t want)
{
	if (want <= 0) return m;
	for (int64_t i = m - 1; i >= 0; --i) {
		const unsigned c = nt4[a[i]], p = i > 0 ? nt4[a[i - 1]] : 4;
		if (!(c < 4 && c == p) && --want == 0) return i;
	}
	return -1;
}
#endif
