/* layer_host.h -- the host scaffolding that the layer libraries share: the error state, the clock, the device guard, device
 * memory that frees itself, the output file of a command and the flush of a text into it, the guard of a handle, the copy of a result list to the
 * caller's device memory, the copy of a walk's results and the exports of the launch tally.  The including file defines LAYER_NAME ("walk", "gfa",
 * "path", ...) first.  Everything here has internal linkage: each library gets code and state of its own, and nothing in here is shared between two
 * of them.  The sequence front end of paths and correct, which needs zlib, is layer_seqs.h. */
#ifndef YAKAMD_LAYER_HOST_H
#define YAKAMD_LAYER_HOST_H
#ifndef LAYER_NAME
#error "define LAYER_NAME, the library's short name in its messages, before layer_host.h"
#endif
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <new>
#include <string>
#include <vector>
#include "yak_amd.h"
#include "yak_amd_walk.h"
#include "../csrc/tally.h"

typedef unsigned long long u64;

namespace {

thread_local char g_err[512];

int fail(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	fprintf(stderr, "[E::yak_amd] %s\n", g_err);
	return -1;
}
#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(LAYER_NAME ": %s -> %s", #x, hipGetErrorString(e_)); } while (0)

/* the message of the library below as ours: it has put it on stderr itself */
inline int fail_below(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); return -1; }

inline double now_ms()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e3 + ts.tv_nsec / 1e6;
}

/* an object's device for a call, and the caller's current device again after it */
struct OnDevice {
	int before = -1;
	explicit OnDevice(int dev) { if (hipGetDevice(&before) != hipSuccess) before = -1; if (before != dev) (void)hipSetDevice(dev); else before = -1; }
	~OnDevice() { if (before >= 0) (void)hipSetDevice(before); }
};

inline unsigned grid_for(u64 n, unsigned threads) { const u64 b = (n + threads - 1) / threads; return (unsigned)(b < 1 ? 1 : b > 2048 ? 2048 : b); }

/* device memory that frees itself; get() allocates what is asked for, need() keeps what is large enough */
struct DevBuf {
	void *p = 0;
	size_t have = 0;
	~DevBuf() { drop(); }
	void drop() { if (p) (void)hipFree(p); p = 0; have = 0; }
	bool get(size_t bytes) { drop(); have = bytes < 256 ? 256 : bytes; if (hipMalloc(&p, have) != hipSuccess) { p = 0; have = 0; } return p != 0; }
	bool need(size_t bytes) { return (p && have >= bytes) || get(bytes + bytes / 8); }
};

/* the output of a command: stdout for no name or "-", else the file; f == 0: it could not be opened */
struct OutFile {
	FILE *f;
	const char *name;
	bool own;
	explicit OutFile(const char *fn) : own(fn && strcmp(fn, "-") != 0) { name = own ? fn : "-"; f = own ? fopen(fn, "wb") : stdout; }
	~OutFile() { if (own && f) fclose(f); }
	bool write(const std::string &t) const { return fwrite(t.data(), 1, t.size(), f) == t.size(); }
	/* after the last write: false if the stream has lost any of them */
	bool finish()
	{
		bool ok = fflush(f) == 0 && !ferror(f);
		if (own) { ok = fclose(f) == 0 && ok; f = 0; }
		return ok;
	}
};

/* a text goes to its output, if it has one, in pieces of 4 MiB; *ok = false once a piece could not be written */
inline void flush(std::string &text, const OutFile *out, bool all, bool *ok)
{
	if (!all && text.size() < (size_t)1 << 22) return;
	if (out && !text.empty()) *ok = out->write(text) && *ok;
	text.clear();
}

/* a handle with a close function that takes none as well, for the length of a command or until close() */
template<class T, void (*Close)(T*)>
struct Guard {
	T *p;
	~Guard() { close(); }
	void close() { Close(p); p = 0; }
};
typedef Guard<yakamd_uwalk_t, yakamd_uwalk_close> WalkGuard;

/* n entries of `each` bytes of a handle's result list into the caller's device memory d of cap entries: n, also where d is none or too small and
 * nothing is copied; -1 with the message.  `none` is what a null handle lacks, `aligned` what must be 16-byte aligned (0: nothing) */
inline int64_t copy_out(bool present, int dev, const void *src, u64 n, u64 each, void *d, int64_t cap, const char *what, const char *none, const char *aligned)
{
	if (!present) return fail("%s: no %s", what, none);
	if (!d || cap < (int64_t)n) return (int64_t)n;
	if (aligned && ((uintptr_t)d & 15) != 0) return fail("%s: %s must be 16-byte aligned", what, aligned);
	if (n == 0) return 0;
	OnDevice on(dev);
	HIPCK(hipMemcpy(d, src, n * each, hipMemcpyDeviceToDevice));
	return (int64_t)n;
}

/* *cap = the power of two at or above what the environment variable asks for, if it is set.  false: it asks for less than n_key slots, none, or
 * more than 2^40; *want is what it asks for */
inline bool slots_from_env(const char *env, u64 n_key, u64 *cap, u64 *want)
{
	const char *sw = getenv(env);
	if (!sw || !*sw) return true;
	*want = strtoull(sw, 0, 10);
	if (*want < n_key || *want < 1 || *want > (u64)1 << 40) return false;
	for (*cap = 1; *cap < *want; *cap <<= 1) {}
	return true;
}

/* the walk's n_u descriptors and n_bases bases into device memory of this library (the buffer of the bases a multiple of `pad` bytes), the
 * descriptors on the host as well.  0; 1: no device memory, the caller says for how much; -1 with the message */
template<class Desc>
int copy_walk(yakamd_uwalk_t *w, u64 n_u, u64 n_bases, u64 pad, DevBuf &desc, DevBuf &bases, std::vector<Desc> &h_desc)
{
	static_assert(sizeof(Desc) == sizeof(yakamd_udesc_t), "a descriptor as declared");
	if (!desc.get(n_u * sizeof(Desc)) || !bases.get((n_bases + pad - 1) / pad * pad)) return 1;
	if (yakamd_uwalk_desc_dev(w, desc.p, (int64_t)n_u) != (int64_t)n_u || yakamd_uwalk_bases_dev(w, bases.p, (int64_t)n_bases) != (int64_t)n_bases)
		return fail_below(yakamd_walk_last_error());
	try { h_desc.resize((size_t)n_u); } catch (const std::bad_alloc&) { return fail(LAYER_NAME ": the descriptors of %llu unitigs do not fit the host's memory", n_u); }
	HIPCK(hipMemcpy(h_desc.data(), desc.p, n_u * sizeof(Desc), hipMemcpyDeviceToHost));
	return 0;
}

/* The launch tally of this library: tally.o is linked into each library, and its table is this library's own behind the version script.  Its path
 * events belong to libyak_amd.so and are not listed */
inline int own_tally_names(const char *const **names)
{
	const char *const *all = 0;
	const int n = yakamd_tally_names(&all);
	if (names) *names = all + YKE_N;
	return n - YKE_N;
}
inline void own_tally_read(uint64_t *out, int n)
{
	std::vector<uint64_t> all((size_t)(n > 0 ? n : 0) + YKE_N);
	yakamd_tally_read(all.data(), (int)all.size());
	for (int i = 0; i < n; ++i) out[i] = all[(size_t)i + YKE_N];
}
#define LAYER_TALLY_EXPORTS(lib) \
	extern "C" int yakamd_##lib##_tally_names(const char *const **names) { return own_tally_names(names); } \
	extern "C" void yakamd_##lib##_tally_read(uint64_t *out, int n) { own_tally_read(out, n); } \
	extern "C" void yakamd_##lib##_tally_reset(void) { yakamd_tally_reset(); }

}   // namespace

#endif
