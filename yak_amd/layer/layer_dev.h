/* layer_dev.h -- the device helpers that walk.hip, gfa.hip and path.hip share: the 16-byte word, the CAS functor of the
 * hash tables, a wave's sum and maximum, the workgroup scan and the tiled additive scan on top of it.  Templates and inline functions only: a library
 * that includes this header gets code of its own and no symbol. */
#ifndef YAKAMD_LAYER_DEV_H
#define YAKAMD_LAYER_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long u64;
typedef ulonglong2 v2;                                            /* 16 bytes: one vector load or store */

enum { LY_WAVE = 64 };

struct DevCas {
	__device__ uint64_t operator()(uint64_t *p, uint64_t expected, uint64_t desired) const { return (uint64_t)atomicCAS(reinterpret_cast<u64*>(p), (u64)expected, (u64)desired); }
};

__device__ inline u64 wave_sum(u64 v)
{
#pragma unroll
	for (int o = LY_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
	return v;                                                      /* lane 0 has the sum */
}
__device__ inline u64 wave_max(u64 v)
{
#pragma unroll
	for (int o = LY_WAVE / 2; o > 0; o >>= 1) { const u64 y = __shfl_down(v, o); v = y > v ? y : v; }
	return v;
}

/* what a scan joins: zero() and (what lies in front, own).  The two sums; path.hip has a segmented one, which does not commute */
struct AddU64 {
	__device__ static u64 zero() { return 0; }
	__device__ u64 operator()(u64 front, u64 own) const { return front + own; }
};
struct AddV2 {
	__device__ static v2 zero() { return make_ulonglong2(0, 0); }
	__device__ v2 operator()(v2 front, v2 own) const { return make_ulonglong2(front.x + own.x, front.y + own.y); }
};
/* the value of the lane o in front; a library with a T of its own adds an overload beside its T */
__device__ inline u64 scan_shfl_up(u64 a, int o) { return __shfl_up(a, o); }
__device__ inline v2 scan_shfl_up(v2 a, int o) { return make_ulonglong2(__shfl_up(a.x, o), __shfl_up(a.y, o)); }

/* what the threads in front of this one hold within the workgroup of THREADS, joined in order, and what the whole workgroup holds */
template<int THREADS, class T, class Join>
__device__ inline void block_scan(const T &own, T *before, T *total)
{
	__shared__ T s_w[THREADS / LY_WAVE];
	const unsigned lane = threadIdx.x & (LY_WAVE - 1), wave = threadIdx.x / LY_WAVE;
	const Join join;
	T inc = own;
#pragma unroll
	for (int o = 1; o < LY_WAVE; o <<= 1) {
		const T y = scan_shfl_up(inc, o);
		if (lane >= (unsigned)o) inc = join(y, inc);
	}
	if (lane == LY_WAVE - 1) s_w[wave] = inc;
	T ex = scan_shfl_up(inc, 1);
	if (lane == 0) ex = Join::zero();
	__syncthreads();
	T front = Join::zero(), all = Join::zero();
#pragma unroll
	for (unsigned w = 0; w < THREADS / LY_WAVE; ++w) {
		const T v = s_w[w];
		if (w < wave) front = join(front, v);
		all = join(all, v);
	}
	__syncthreads();                                               /* the next call writes s_w again */
	*before = join(front, ex);
	*total = all;
}

/* The exclusive scan of a[0 .. n) in place by three launches: tiles of THREADS * ITEMS, their sums scanned by one workgroup.
 * tsum[tile] = the sum of a[tile * THREADS * ITEMS ..]; one workgroup per tile, a thread ITEMS consecutive entries */
template<int THREADS, int ITEMS, class T, class Add>
__device__ inline void tile_sum(const T *a, u64 n, T *tsum)
{
	const u64 i0 = (u64)blockIdx.x * (THREADS * ITEMS) + (u64)threadIdx.x * ITEMS;
	const Add add;
	T own = Add::zero(), before, total;
#pragma unroll
	for (int i = 0; i < ITEMS; ++i) if (i0 + i < n) own = add(own, a[i0 + i]);
	block_scan<THREADS, T, Add>(own, &before, &total);
	if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

/* the exclusive scan of tsum[0 .. m) in place, its sum in tsum[m]: one workgroup of THREADS, each thread a contiguous slice */
template<int THREADS, class T, class Add>
__device__ inline void tile_scan(T *tsum, u64 m)
{
	const u64 per = (m + THREADS - 1) / THREADS, lo = (u64)threadIdx.x * per < m ? (u64)threadIdx.x * per : m, hi = lo + per < m ? lo + per : m;
	const Add add;
	T own = Add::zero(), before, total;
	for (u64 i = lo; i < hi; ++i) own = add(own, tsum[i]);
	block_scan<THREADS, T, Add>(own, &before, &total);
	for (u64 i = lo; i < hi; ++i) { const T v = tsum[i]; tsum[i] = before; before = add(before, v); }
	if (threadIdx.x == 0) tsum[m] = total;
}

/* a[] becomes its exclusive scan, tile by tile on top of the scanned tile sums */
template<int THREADS, int ITEMS, class T, class Add>
__device__ inline void scan_apply(T *a, u64 n, const T *tsum)
{
	const u64 i0 = (u64)blockIdx.x * (THREADS * ITEMS) + (u64)threadIdx.x * ITEMS;
	const Add add;
	T it[ITEMS], own = Add::zero(), before, total;
#pragma unroll
	for (int i = 0; i < ITEMS; ++i) it[i] = i0 + i < n ? a[i0 + i] : Add::zero();
#pragma unroll
	for (int i = 0; i < ITEMS; ++i) own = add(own, it[i]);             /* behind the loads: they are in flight together */
	block_scan<THREADS, T, Add>(own, &before, &total);
	before = add(tsum[blockIdx.x], before);
#pragma unroll
	for (int i = 0; i < ITEMS; ++i) if (i0 + i < n) { a[i0 + i] = before; before = add(before, it[i]); }
}

#endif
