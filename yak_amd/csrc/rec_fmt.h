/* rec_fmt.h -- what a buffer of level-1 records holds; it travels as `const void *` beside its RecFmt.  A Chunk2 holds the
 * first two, and the level-2 kernels compare Chunk2::fmt with these values.  Plain C++, a header of its own: yk_device.h gives it to the kernels and
 * the engine, count_plan.h reads it without the HIP runtime's headers.  The layouts and their sizes are in yk_device.h (Rec, YK_R8_*, yk_rec_bytes). */
#ifndef YK_REC_FMT_H
#define YK_REC_FMT_H
enum RecFmt {
	YK_FMT_POS = 0,                      /* Rec {hash, position}, 16 bytes */
	YK_FMT_TAGGED = 1,                   /* the tagged level-1 record, 8 bytes */
	YK_FMT_HASH = 2,                     /* the bare hash, 8 bytes */
	YK_FMT_HASH_RNG = 3                  /* the hash with the sub-table's own bits (the bucket says them) replaced by the top bits of its home-slot product: k_img_count_own's range test, 8 bytes */
};
#endif
