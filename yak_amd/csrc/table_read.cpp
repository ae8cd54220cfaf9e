/*
 * table_read.cpp -- what the commands that read a resident table's stored keys share (dump, print, inspect on resident tables, hetmers, unitigs):
 * the owner of one staged range of whole sub-tables, the cut of a range of sub-tables by the shard that owns them, the range rule over a
 * context's sizes, and the refusals of the commands that need the whole table as one image.
 */
#include "engine_int.h"

int StagedRange::stage(yakamd_ctx *c, int lo, int hi, const std::vector<u64> *off, const char *what, const char *verb)
{
	drop();
	if (dev != c->dev) d_off.drop();                              /* (a buffer of another device is not this range's to fill) */
	dev = c->dev;
	if (yk_ctx_dump_image_dev(c, lo, hi, &d_img, &n_words) != 0) return -1;
	if (!off) return 0;
	if (n_words != off->back() + (u64)(hi - lo)) return fail("%s: the table changed while it was %s", what, verb);
	if (!d_off.fit(off->size() * 8) || yakamd_memcpy_h2d(d_off.p, off->data(), off->size() * 8) != 0)
		return fail("%s: no device memory for %zu offsets", what, off->size());
	return 0;
}

void StagedRange::drop()
{
	if (!d_img) return;
	(void)hipSetDevice(dev);
	yk_pool_release(d_img);
	d_img = 0; n_words = 0;
}

std::vector<TableRange> yk_ctx_ranges(yakamd_ctx *c, int lo, int hi, int64_t budget, bool keep_empty)
{
	return table_ranges(lo, hi, [c](int p) { return (u64)c->h_count[p]; }, budget, keep_empty);
}

bool yk_table_pieces(const yak_ch_t *h, int lo, int hi, const char *what, std::vector<TablePiece> *out)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	out->clear();
	if (!h || e->magic != EXT_MAGIC) { fail("%s: not an engine table", what); return false; }
	if (lo < 0 || hi < lo || hi > 1 << h->pre) { fail("%s: sub-tables [%d, %d) of %d", what, lo, hi, 1 << h->pre); return false; }
	const int n_sh = e->n_sub > 1 ? e->n_sub : 1;
	for (int r = 0; r < n_sh; ++r) {
		yak_ch_t *s = e->n_sub > 1 ? e->sub[r] : (yak_ch_t*)h;
		std::vector<yakamd_ctx*> eng;
		if (yk_inspect_engines(s, &eng)) return false;               /* (an engine table, out of a pass) */
		const int a = std::max(eng[0]->plo, lo), b = std::min(eng[0]->phi, hi);
		if (a < b) out->push_back(TablePiece{ eng[0], a, b });
	}
	return true;
}

ImageState yk_image_state(const yak_ch_t *h)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	const bool multi = h && e->magic == EXT_MAGIC && e->n_sub > 1;
	ImageState s;
	s.c = multi ? ctx_of(e->sub[0]) : ctx_of(h);
	s.sharded = multi || (s.c && (s.c->plo != 0 || s.c->phi != s.c->P));
	s.in_pass = s.c && s.c->in_pass;
	for (int r = 1; multi && r < e->n_sub; ++r) { yakamd_ctx *o = ctx_of(e->sub[r]); s.in_pass = s.in_pass || (o && o->in_pass); }
	return s;
}

yakamd_ctx *yk_whole_image_ctx(const yak_ch_t *h, int min_cnt, const char *what, const char *no_gpu, const char *even_k)
{
	if (yakamd_device_count() < 1) { fail("%s: no gfx950 GPU visible: %s", what, no_gpu); return 0; }
	const ImageState s = yk_image_state(h);
	if (!s.c) fail("%s: not an engine table", what);
	else if (!(h->k & 1)) fail("%s: k = %d is even: %s", what, h->k, even_k);
	else if (h->k >= 32) fail("%s: k = %d: k must be below 32 (a stored key inverts to its k-mer for k below 32 only, reference htab.c:359)", what, h->k);
	else if (min_cnt < 1 || min_cnt > YAK_N_COUNTS - 1) fail("%s: min_cnt %d is outside [1, %d]", what, min_cnt, YAK_N_COUNTS - 1);
	else if (s.in_pass) fail("%s during an open pass", what);
	else if (s.sharded) fail("%s: " YK_MSG_SHARDED, what);
	else return s.c;
	return 0;
}
