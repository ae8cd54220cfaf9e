/* dev_buf.h -- owners of device-pool memory: DevBuf<T>, one allocation that lives with a scope or a struct, and DevVec<T>, a buffer with a
 * capacity that only grows.  Nothing here but the three declarations below: a host program can compile this header against a pool of its own
 * (tests/tools/dev_buf_check.cpp). */
#ifndef YK_DEV_BUF_H
#define YK_DEV_BUF_H
#include <stddef.h>
#include <utility>

void *yk_pool_alloc(size_t bytes, bool plain);              /* pool.cpp */
void yk_pool_free(void *p);
int yk_set_error(const char *fmt, ...);                      /* returns -1 */

template <class T> static int dmalloc(T **p, size_t n)
{
	if (n == 0) n = 1;
	*p = (T*)yk_pool_alloc(n * sizeof(T), false);
	if (!*p) return yk_set_error("device allocation of %zu bytes failed", n * sizeof(T));
	return 0;
}
template <class T> static void dfree(T *&p) { if (p) { yk_pool_free((void*)p); p = 0; } }

/* one pool allocation owned by a scope or a struct: freed by its destructor or by reset(); release() hands the pointer to whoever frees it next */
template <class T> class DevBuf {
	T *p_ = 0;
public:
	DevBuf() = default;
	explicit DevBuf(T *p) : p_(p) {}
	DevBuf(DevBuf &&o) noexcept : p_(o.release()) {}
	DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.release(); } return *this; }   /* (and no copies) */
	~DevBuf() { reset(); }
	int alloc(size_t n) { reset(); return dmalloc(&p_, n); }
	void reset() { dfree(p_); }
	T *release() { T *p = p_; p_ = 0; return p; }
	T *get() const { return p_; }
	operator T *() const { return p_; }
};

/* a buffer that is asked for room again and again and only ever grows.  reserve(n) allocates exactly n elements -- the growth rule is the
 * caller's, in the n it asks for -- and frees the old buffer first: the two never exist together.  A failed allocation leaves no buffer and
 * no capacity */
template <class T> class DevVec {
	DevBuf<T> b_;
	size_t cap_ = 0;
public:
	DevVec() = default;
	DevVec(DevVec &&o) noexcept : b_(std::move(o.b_)), cap_(o.cap_) { o.cap_ = 0; }
	DevVec &operator=(DevVec &&o) noexcept { if (this != &o) { b_ = std::move(o.b_); cap_ = o.cap_; o.cap_ = 0; } return *this; }
	int reserve(size_t n)
	{
		if (n <= cap_) return 0;
		cap_ = 0;
		if (b_.alloc(n)) return -1;
		cap_ = n;
		return 0;
	}
	void reset() { b_.reset(); cap_ = 0; }
	T *get() const { return b_.get(); }
	size_t cap() const { return cap_; }
	operator T *() const { return b_.get(); }
};
#endif
