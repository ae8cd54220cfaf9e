/* seg_sort_tile.h -- the offset arithmetic of one tile of k_seg_sort_pass (kern_layout.inc), free of HIP so that tests/tools/seg_sort_check.cpp can
 * run whole sorts through it on the CPU.
 *
 * A pass sorts a segment stably by one 8-bit digit of T.  A workgroup of NT threads takes the segment a tile at a time.  The tile is split
 * wave-major: wave w owns the sst_per_thread(NT) x 64 consecutive elements from w x 64 x E on and ranks them 64 at a time, so (wave, round, lane)
 * order is source order.  Per digit d the kernel keeps
 *   run[d]    where the digit's next element goes in the segment (the exclusive scan of the histogram, advanced tile by tile)
 *   wc[w][d]  what wave w holds of d; sst_wave_prefix turns the column into an exclusive prefix over the waves and returns the tile's total
 *   start[d]  where the digit's run starts inside the tile: the exclusive scan of those totals over the digits
 * An element of digit d, wave w, rank k among its wave's d goes to sst_lds_pos = start[d] + wc[w][d] + k of an LDS copy of the tile.  The copy
 * is stored in index order, element i of it to sst_global = segment + run[d] + (i - start[d]): consecutive lanes write consecutive addresses
 * of one digit's run.  sst_base keeps run[d] - start[d] (modulo 2^32: the sum with i is a true offset again), so a store needs one table. */
#ifndef YK_SEG_SORT_TILE_H
#define YK_SEG_SORT_TILE_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SST_FN __host__ __device__ static inline
#else
#define SST_FN static inline
#endif

#define SST_NBIN 256

/* elements per thread and tile: the LDS copy of a 1024-thread tile (8 bytes x 4096, keys and times one after the other) leaves room for two
 * workgroups per CU next to the per-wave counters */
SST_FN constexpr int sst_per_thread(int nt) { return nt >= 1024 ? 4 : 8; }
SST_FN constexpr int sst_tile(int nt) { return nt * sst_per_thread(nt); }

SST_FN uint32_t sst_digit(uint64_t t, int shift) { return (uint32_t)(t >> shift) & (SST_NBIN - 1); }

/* offset in the segment of the element that lane `lane` of wave `wave` takes in round r of the tile at `tile` */
SST_FN uint64_t sst_src_index(uint64_t tile, int wave, int r, int lane, int e) { return tile + (uint64_t)wave * (64 * e) + (uint64_t)r * 64 + lane; }

/* digit d's column of the per-wave counts wc[nwv][SST_NBIN] -> exclusive prefix over the waves; returns the tile's count of d */
SST_FN uint32_t sst_wave_prefix(uint32_t *wc, int nwv, int d)
{
	uint32_t run = 0;
	for (int w = 0; w < nwv; ++w) { const uint32_t c = wc[w * SST_NBIN + d]; wc[w * SST_NBIN + d] = run; run += c; }
	return run;
}

SST_FN uint32_t sst_lds_pos(uint32_t start_d, uint32_t wave_prefix, uint32_t rank) { return start_d + wave_prefix + rank; }
SST_FN uint32_t sst_base(uint32_t run_d, uint32_t start_d) { return run_d - start_d; }
SST_FN uint64_t sst_global(uint64_t seg, uint32_t base_d, uint32_t i) { return seg + (uint32_t)(base_d + i); }

/* the digit whose histogram row a pass with this shift uses, of the sst_n_digits(tbits) rows its sort's first pass counted */
SST_FN int sst_n_digits(int tbits) { return (tbits + 7) / 8; }
#define SST_MAX_DIGITS 8
SST_FN uint64_t sst_hist_row(uint64_t seg_no, int n_dig, int dig) { return ((uint64_t)seg_no * n_dig + dig) * SST_NBIN; }

#endif
