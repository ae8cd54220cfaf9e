/* engine_table.cpp -- operations on a whole table image: histogram, setcnt and clear, the rebuilds (shrink, subtract, isec), the khashl resizes
 * (tighten, merge pre-size, resize to saved capacities), the listings (hashes, .yak image), the count step of a sum, load and inc. */
#include "engine_int.h"

int yk_ctx_hist(yakamd_ctx *c, int64_t *cnt1024)
{
	HIPCK(hipSetDevice(c->dev));
	DevBuf<u64> d_h;
	if (d_h.alloc(1024)) return -1;
	HIPCK(hipMemsetAsync(d_h, 0, 1024 * 8, c->st));
	yk_launch_img_hist(img_view(c), c->n_slots, d_h, c->st);
	const hipError_t e = hipMemcpyAsync(cnt1024, d_h, 1024 * 8, hipMemcpyDeviceToHost, c->st);
	const hipError_t e2 = hipStreamSynchronize(c->st);
	return e == hipSuccess && e2 == hipSuccess ? 0 : fail("hist: %s", hipGetErrorString(e != hipSuccess ? e : e2));
}

int yk_ctx_setcnt(yakamd_ctx *c, int cnt)
{
	HIPCK(hipSetDevice(c->dev));
	yk_launch_img_setcnt(img_view(c), c->n_slots, (u32)cnt & 1023u, c->st);
	HIPCK(hipStreamSynchronize(c->st));
	c->host_valid = false;
	yk_image_touched(c);
	return 0;
}

/* The clear is only noted: k_img_clear runs when something next reads or writes the image (img_view -> yk_image_settle), on the same stream and so
 * in the same order as if it had run here.  The count pass over the input of the pass before is the one caller that takes the note over instead
 * (yakamd_count_retained: clear and count in one sweep).  The precedent is the filter k_lc2 does not write back (bf_deferred) */
int yk_ctx_clear(yakamd_ctx *c)
{
	c->clear_pending = true;
	c->host_valid = false;
	return 0;
}

int yk_image_settle(yakamd_ctx *c)
{
	static std::mutex mu;                                      /* readers on several threads (lookups): the first one clears, the others wait for it */
	std::lock_guard<std::mutex> lk(mu);
	if (!c->clear_pending) return 0;
	int cur = c->dev;                                          /* (the image of another table of a command -- subtract, isec -- may live on another device) */
	(void)hipGetDevice(&cur);
	if (cur != c->dev) HIPCK(hipSetDevice(c->dev));
	yk_launch_img_clear(img_view_pending(c), c->n_slots, c->st);
	const hipError_t e = hipStreamSynchronize(c->st);          /* as yak_ch_clear always did: readers on other streams see the zeros */
	c->clear_pending = false;
	if (cur != c->dev) (void)hipSetDevice(cur);
	return e == hipSuccess ? 0 : fail("clear: %s", hipGetErrorString(e));
}

/* reference htab.c:180-208 */
/* htab.c:171-197 (shrink), 287-347 (subtract / isec): per sub-table, a new set resized for the old
 * key count receives, in old slot order, the keys that pass the test.  which: 0 count range only,
 * 1 and absent from `other`, 2 and present in `other` */
static int rebuild(yakamd_ctx *c, int cmin, int cmax, int which, yakamd_ctx *other, u64 *tot)
{
	HIPCK(hipSetDevice(c->dev));
	const int P = c->P;
	if (other && (other->pre != c->pre || other->k != c->k)) return fail("tables of different k / prefix length");
	const ImgView ov = other ? img_view(other) : img_view(c);
	std::vector<u32> m(P), init(P);
	std::vector<u64> seg_off(P + 1, 0);
	DevBuf<u64> d_kc, d_segoff; DevBuf<u32> d_segcnt;
	const int RG = yk_shrink_shares();                            /* workgroups per sub-table */
	std::vector<u32> mr((size_t)P * RG);
	if (d_segcnt.alloc((size_t)P * RG) || d_segoff.alloc(P + 1)) return -1;
	yk_launch_shrink_count(img_view(c), P, cmin, cmax, which, ov, d_segcnt, c->st, 1);
	HIPCK(hipMemcpyAsync(mr.data(), d_segcnt, mr.size() * 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	for (int p = 0; p < P; ++p) {
		m[p] = 0;
		for (int g = 0; g < RG; ++g) m[p] += mr[(size_t)p * RG + g];
		seg_off[p + 1] = seg_off[p] + m[p]; init[p] = kh_bits_for(c->h_count[p]);
	}
	if (d_kc.alloc(seg_off[P])) return -1;
	HIPCK(hipMemcpyAsync(d_segoff, seg_off.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
	yk_launch_shrink_scatter(img_view(c), P, cmin, cmax, which, ov, d_segoff, d_kc, c->st, d_segcnt);
	EvTimer tm(c->st);
	const int r = yk_run_replay(c, m, d_kc, 0, 0, &init, true);
	c->st_last.ms_shrink = tm.stop();
	if (r) return r;
	*tot = c->img_keys_total;
	return 0;
}

int yk_ctx_shrink(yakamd_ctx *c, int cmin, int cmax, u64 *tot) { return rebuild(c, cmin, cmax, 0, 0, tot); }
int yk_ctx_subtract(yakamd_ctx *c, yakamd_ctx *other, u64 *tot) { return rebuild(c, 0, 1023, 1, other, tot); }
int yk_ctx_isec(yakamd_ctx *c, yakamd_ctx *other, u64 *tot) { return rebuild(c, 0, 1023, 2, other, tot); }

/* khashl resize of every sub-table whose entry in new_bits differs from YK_NOCAP-as-"leave alone"
 * (new_bits[p] == 0xfffffffe); the table image moves to a fresh arena */
#define YK_LEAVE 0xfffffffeu
static int resize_tables(yakamd_ctx *c, const std::vector<u32> &new_bits)
{
	HIPCK(hipSetDevice(c->dev));
	if (yk_image_settle(c)) return -1;
	const int P = c->P;
	std::vector<ResizeTask> tasks(P);
	std::vector<u64> new_off(P);
	std::vector<u32> bits_after(P);
	u64 tot = 0;
	for (int p = 0; p < P; ++p) {
		ResizeTask &t = tasks[p];
		t.old_bits = c->h_bits[p]; t.old_off = c->h_off[p]; t.pad = 0;
		t.rehash = new_bits[p] != YK_LEAVE;
		t.new_bits = t.rehash ? new_bits[p] : c->h_bits[p];
		bits_after[p] = t.new_bits;
		const u64 n = t.old_bits == YK_NOCAP ? 0 : (u64)1 << t.old_bits, N = t.new_bits == YK_NOCAP ? 0 : (u64)1 << t.new_bits;
		t.new_off = new_off[p] = tot;
		tot += std::max<u64>(32, std::max(n, N));
	}
	DevBuf<ResizeTask> d_tasks; DevBuf<u32> su, nu; DevBuf<u64> nk;
	if (nk.alloc(tot) || nu.alloc(tot / 32) || su.alloc(tot / 32) || d_tasks.alloc(P)) return -1;
	HIPCK(hipMemsetAsync(nk, 0xff, tot * 8, c->st));
	HIPCK(hipMemsetAsync(nu, 0, tot / 8, c->st));
	HIPCK(hipMemcpyAsync(d_tasks, tasks.data(), P * sizeof(ResizeTask), hipMemcpyHostToDevice, c->st));
	yk_launch_resize(d_tasks, P, c->d_keys, c->d_used, nk, nu, su, c->st);
	HIPCK(hipStreamSynchronize(c->st));
	su.reset(); d_tasks.reset();
	c->h_bits = bits_after;
	return yk_image_commit(c, std::move(nk), std::move(nu), tot, new_off);
}

/* new_bits of khashl's resize(want) on a set of (cap, count), or YK_LEAVE when it refuses (khashl.h:155-160) */
static u32 resize_target(u32 count, u32 want)
{
	const u32 nb = kh_bits_for(want);
	const u64 N = (u64)1 << nb;
	return count > (N >> 1) + (N >> 2) ? YK_LEAVE : nb;
}

/* htab.c:102-110: sub-tables filled to less than a third are resized to 3 x their key count */
int yk_ctx_tighten(yakamd_ctx *c)
{
	const int P = c->P;
	std::vector<u32> nb(P, YK_LEAVE);
	bool any = false;
	for (int p = 0; p < P; ++p) {
		const u64 cap = c->h_bits[p] == YK_NOCAP ? 0 : (u64)1 << c->h_bits[p];
		if ((u64)c->h_count[p] * 3 < cap) { nb[p] = resize_target(c->h_count[p], c->h_count[p] * 3); any = any || nb[p] != YK_LEAVE; }
	}
	return any ? resize_tables(c, nb) : 0;
}

/* htab.c:262-266: before a merge, grow sub-table p for count0 + count1 keys at 75 % load */
int yk_ctx_merge_presize(yakamd_ctx *c, yakamd_ctx *other)
{
	const int P = c->P;
	std::vector<u32> nb(P, YK_LEAVE);
	bool any = false;
	/* only the sub-tables both sides own: a shard of a table sharded over prefix ranges says nothing about the others (each sub-table
	 * must meet its one pre-resize with the true key count of the other side) */
	for (int p = std::max(c->plo, other->plo); p < std::min(c->phi, other->phi); ++p) {
		const u64 cap = c->h_bits[p] == YK_NOCAP ? 0 : (u64)1 << c->h_bits[p];
		const u64 want = ((u64)c->h_count[p] + other->h_count[p]) * 4 / 3 + 1;
		if (want > cap) { nb[p] = resize_target(c->h_count[p], (u32)want); any = any || nb[p] != YK_LEAVE; }
	}
	return any ? resize_tables(c, nb) : 0;
}

/* keys of `c` with cmin <= count <= cmax, sub-table by sub-table in slot order, as full hashes +
 * list positions on the device (caller frees both with yakamd_dev_free-compatible pool_free); with d_cnt, their 10-bit counts as well */
int yk_ctx_list_hashes(yakamd_ctx *c, int cmin, int cmax, u64 **d_hash, u32 **d_t, u64 *n, unsigned short **d_cnt)
{
	HIPCK(hipSetDevice(c->dev));
	const int P = c->P;
	std::vector<u32> m(P);
	std::vector<u64> seg_off(P + 1, 0);
	DevBuf<u32> t; DevBuf<u64> hash, d_kc, d_segoff; DevBuf<u32> d_segcnt; DevBuf<unsigned short> cnt;
	*d_hash = 0; *d_t = 0;
	if (d_cnt) *d_cnt = 0;
	if (d_segcnt.alloc(P) || d_segoff.alloc(P + 1)) return -1;
	yk_launch_shrink_count(img_view(c), P, cmin, cmax, 0, img_view(c), d_segcnt, c->st);
	HIPCK(hipMemcpyAsync(m.data(), d_segcnt, P * 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	for (int p = 0; p < P; ++p) seg_off[p + 1] = seg_off[p] + m[p];
	*n = seg_off[P];
	if (d_kc.alloc(seg_off[P]) || hash.alloc(seg_off[P]) || t.alloc(seg_off[P]) || (d_cnt && cnt.alloc(seg_off[P]))) return -1;
	HIPCK(hipMemcpyAsync(d_segoff, seg_off.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
	yk_launch_shrink_scatter(img_view(c), P, cmin, cmax, 0, img_view(c), d_segoff, d_kc, c->st);
	yk_launch_keys_to_hashes(d_kc, d_segoff, P, c->pre, hash, t, c->st, d_cnt ? cnt.get() : 0);
	HIPCK(hipStreamSynchronize(c->st));
	*d_hash = hash.release(); *d_t = t.release();
	if (d_cnt) *d_cnt = cnt.release();
	return 0;
}

/* yakamd_ch_sum's count step (k_img_add_counts): entry i of a listing of another table's keys, d_hash[i] with count d_cnt[i] >= 1, which a create
 * pass has just put into `c`, gets min(1023, its count here + d_cnt[i] - 1); the entries of sub-tables outside c's prefix range are skipped.  The
 * listing may lie on a peer device.  Fails, after the kernel, when a listed key was not found */
int yk_ctx_add_counts(yakamd_ctx *c, const u64 *d_hash, const unsigned short *d_cnt, u64 n)
{
	if (c->in_pass) return fail("yk_ctx_add_counts during an open pass");
	if (n == 0) return 0;
	HIPCK(hipSetDevice(c->dev));
	DevBuf<u32> d_missing;
	u32 missing = 0;
	if (d_missing.alloc(1)) return -1;
	HIPCK(hipMemsetAsync(d_missing, 0, 4, c->st));
	yk_image_touched(c);
	yk_launch_img_add_counts(d_hash, d_cnt, n, img_view(c), c->plo, c->phi, d_missing, c->st);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpyAsync(&missing, d_missing, 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	c->host_valid = false;
	if (missing) return fail("sum: a listed key is not in the table after its create pass: the counts were not all added");
	return 0;
}

/* the .yak bytes of sub-tables [lo, hi) -- per sub-table capacity and size (4 bytes each) and the stored keys in ascending slot order,
 * htab.c:385-389 -- put together on the device: *d_img (pool memory: yk_pool_release) holds *n_words 8-byte words, ready on the table's stream */
int yk_ctx_dump_image_dev(yakamd_ctx *c, int lo, int hi, u64 **d_img, u64 *n_words)
{
	HIPCK(hipSetDevice(c->dev));
	const int P = c->P, n = hi - lo;
	*d_img = 0; *n_words = 0;
	if (lo < 0 || hi > P || n <= 0) return fail("yk_ctx_dump_image_dev: sub-tables [%d, %d) of %d", lo, hi, P);
	std::vector<u64> seg_off(P + 1, ~0ull), head(2 * (size_t)n);     /* ~0: a sub-table outside [lo, hi) is skipped */
	u64 at = 0;
	for (int p = lo; p < hi; ++p) {
		head[p - lo] = at;
		head[n + p - lo] = (u64)(c->h_bits[p] == YK_NOCAP ? 0 : 1u << c->h_bits[p]) | (u64)c->h_count[p] << 32;
		seg_off[p] = ++at;
		at += c->h_count[p];
	}
	DevBuf<u64> img, d_head, d_segoff;
	if (d_segoff.alloc(P + 1) || d_head.alloc(2 * (size_t)n) || img.alloc(at)) return -1;
	HIPCK(hipMemcpyAsync(d_segoff, seg_off.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemcpyAsync(d_head, head.data(), head.size() * 8, hipMemcpyHostToDevice, c->st));
	yk_launch_shrink_scatter(img_view(c), P, 0, 1023, 0, img_view(c), d_segoff, img, c->st);
	yk_launch_put_u64(d_head, d_head + n, (u32)n, img, c->st);
	HIPCK(hipStreamSynchronize(c->st));                            /* (the two small host arrays and the offsets go away with this call) */
	*d_img = img.release(); *n_words = at;
	return 0;
}

/* khashl resize(want[p]) on every sub-table (htab.c:441 on an existing table): same size re-places in place */
int yk_ctx_resize_to(yakamd_ctx *c, const uint32_t *want)
{
	const int P = c->P;
	std::vector<u32> nb(P, YK_LEAVE);
	bool any = false;
	for (int p = 0; p < P; ++p) { nb[p] = resize_target(c->h_count[p], want[p]); any = any || nb[p] != YK_LEAVE; }
	return any ? resize_tables(c, nb) : 0;
}

/* reference htab.c:441-447: resize each sub-table to its saved capacity, then put in file order */
int yk_ctx_load(yakamd_ctx *c, const uint32_t *caps, const uint32_t *sizes, const uint64_t *keys)
{
	HIPCK(hipSetDevice(c->dev));
	const int P = c->P;
	std::vector<u32> m(P), init(P);
	u64 tot = 0;
	for (int p = 0; p < P; ++p) { m[p] = sizes[p]; init[p] = kh_bits_for(caps[p]); tot += sizes[p]; }
	DevBuf<u64> d_kc;
	if (d_kc.alloc(tot)) return -1;
	HIPCK(hipMemcpyAsync(d_kc, keys, tot * 8, hipMemcpyHostToDevice, c->st));
	return yk_run_replay(c, m, d_kc, 0, 0, &init, true);
}

/* reference htab.c:80-91: saturating ++ of one stored k-mer; -1 if absent.  One single-lane kernel; a valid host
 * mirror is patched in place instead of being refreshed */
int yk_ctx_inc(yakamd_ctx *c, u64 hash, int *count)
{
	if (c->in_pass) return fail("yak_ch_inc during an open pass");
	HIPCK(hipSetDevice(c->dev));
	u64 out[2];
	yk_image_touched(c);
	yk_launch_img_inc(img_view(c), hash, c->d_counters, c->st);
	HIPCK(hipMemcpyAsync(out, c->d_counters, 16, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (out[0] == ~0ull) { *count = -1; return 0; }
	*count = (int)out[1];
	if (c->host_valid && c->hm_keys) c->hm_keys[out[0]] = (c->hm_keys[out[0]] & ~1023ull) | out[1];
	return 0;
}
