/*
 * yak_graph.cpp -- `yak-amd unitigs` (not in the reference): the de Bruijn graph the k-mers of a count table span, its
 * compacted form and its unitigs.  yakamd_graph_open() probes the resident table for every node's eight possible neighbours once (k_graph_edges,
 * kern_graph.inc) and keeps one edge byte per arena slot, the rank directory that turns a slot into its listing index (k_graph_rank) and the tallies;
 * yakamd_graph_nodes_dev() writes the records of a range of sub-tables in listing order, each with the listing indices its two sides are linked to
 * (k_graph_link: one more probe per side of one edge).  yakamd_unitigs() pulls the records to the host in ranges of whole sub-tables and walks them
 * there (unitig_walk.h).  The table is not modified and no host mirror of it is built.
 */
#include <new>
#include "engine_int.h"
#include "unitig_walk.h"

static_assert(sizeof(yakamd_gnode_t) == 32 && sizeof(ug_node_t) == 32, "a graph record is 32 bytes");

struct yakamd_graph {
	yak_ch_t *h;
	yakamd_ctx *c;
	int min_cnt;
	std::vector<u64> tile0, key0;                                  /* [P + 1]: the tiles / stored keys of the sub-tables before p */
	DevBuf<u64> d_dir;                                             /* tile0, then key0 */
	DevBuf<uint8_t> d_edges;
	DevBuf<u32> d_wrank;
	DevBuf<u64> d_tally;
	const u64 *keys_then; u64 slots_then, total_then;              /* the image the scratch describes */
	yakamd_gstat_t st;
	double ms_edges, ms_rank, ms_link;
	~yakamd_graph() { if (c) (void)hipSetDevice(c->dev); }         /* the scratch goes back to the pool of the table's device */
};

namespace {

const int64_t GR_BATCH_DEFAULT = (int64_t)1 << 24;
double g_unitigs_ms[4];                                           /* the last yakamd_unitigs call: graph, records, walk, text */

/* a later call on an open graph: the pass and the image are looked at again */
int gr_still(yakamd_graph_t *g, const char *what)
{
	if (!g) return fail("%s: no graph", what);
	yakamd_ctx *c = g->c;
	if (c->in_pass) return fail("%s during an open pass", what);
	if (c->d_keys != g->keys_then || c->n_slots != g->slots_then || c->img_keys_total != g->total_then)
		return fail("%s: the table changed after yakamd_graph_open", what);
	return 0;
}

int gr_launch(yakamd_graph_t *g, int what, u64 t_lo, u64 t_hi, void *out, u64 out_key0, u64 out_n)
{
	yakamd_ctx *c = g->c;
	const int inflight = (int)yk_knob("YAKAMD_GRAPH_INFLIGHT", 4);   /* two rounds of four probes: 14.5 ms against 15.1 ms with all eight together (profiles/graph_timing.txt) */
	const int grid = (int)std::max<int64_t>(0, std::min<int64_t>(yk_knob("YAKAMD_GRAPH_GRID", 0), 1 << 20));
	return yk_launch_graph(what, inflight, grid, g->d_dir, g->d_dir + c->P + 1, g->d_edges, g->d_wrank, g->d_tally, t_lo, t_hi, c->n_slots, c->P, g->min_cnt,
	                       out, out_key0, out_n, img_view(c), c->st);
}

int gr_build(yakamd_graph_t *g)
{
	yakamd_ctx *c = g->c;
	const int P = c->P;
	HIPCK(hipSetDevice(c->dev));
	const u64 T = yk_graph_tile();
	g->tile0.assign(P + 1, 0); g->key0.assign(P + 1, 0);
	for (int p = 0; p < P; ++p) {
		const u64 cap = c->h_bits[p] == YK_NOCAP ? 0 : 1ull << c->h_bits[p];
		if (cap && (c->h_off[p] & 31)) return fail("graph: sub-table %d does not start on a word of the bitmap", p);
		g->tile0[p + 1] = g->tile0[p] + (cap + T - 1) / T;
		g->key0[p + 1] = g->key0[p] + c->h_count[p];
	}
	if (g->key0[P] != c->img_keys_total) return fail("graph: the sub-tables hold %llu keys, the table %llu", (unsigned long long)g->key0[P], (unsigned long long)c->img_keys_total);
	std::vector<u64> dir(g->tile0);
	dir.insert(dir.end(), g->key0.begin(), g->key0.end());
	if (g->d_dir.alloc(dir.size()) || g->d_edges.alloc((size_t)c->n_slots) || g->d_wrank.alloc((size_t)(c->n_slots / 32 + 1)) || g->d_tally.alloc(32))
		return fail("graph: no device memory for %.1f MB of scratch", c->n_slots * 1.125 / 1e6);
	HIPCK(hipMemcpyAsync(g->d_dir, dir.data(), dir.size() * 8, hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemsetAsync(g->d_tally, 0, 32 * 8, c->st));
	const bool timed = getenv("YAKAMD_VERBOSE") != 0 || yk_knob("YAKAMD_GRAPH_TIMED", 0) != 0;
	double t0 = now_ms();
	if (gr_launch(g, 0, 0, g->tile0[P], 0, 0, 0)) return fail("graph: the edge kernel did not launch");
	if (timed) { HIPCK(hipStreamSynchronize(c->st)); g->ms_edges = now_ms() - t0; t0 = now_ms(); }
	if (gr_launch(g, 1, 0, g->tile0[P], 0, 0, 0)) return fail("graph: the rank kernel did not launch");
	if (timed) { HIPCK(hipStreamSynchronize(c->st)); g->ms_rank = now_ms() - t0; t0 = now_ms(); }
	if (gr_launch(g, 2, 0, g->tile0[P], 0, 0, 0)) return fail("graph: the link kernel did not launch");
	u64 tally[32];
	HIPCK(hipMemcpyAsync(tally, g->d_tally, sizeof tally, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (timed) g->ms_link = now_ms() - t0;
	yakamd_gstat_t &s = g->st;
	memset(&s, 0, sizeof s);
	s.n_key = g->key0[P];
	for (int l = 0; l < 5; ++l)
		for (int r = 0; r < 5; ++r) { const u64 v = tally[l * 5 + r]; s.deg[l][r] = v; s.n_node += v; s.n_arc += v * (u64)(l + r); }
	s.n_linked_side = tally[25];
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] graph: %llu keys, %llu nodes, %llu arcs; edges %.2f ms, rank %.2f ms, links %.2f ms\n", (unsigned long long)s.n_key,
		        (unsigned long long)s.n_node, (unsigned long long)s.n_arc, g->ms_edges, g->ms_rank, g->ms_link);
	return 0;
}

int64_t gr_batch(int64_t dflt)
{
	const int64_t b = yk_knob("YAKAMD_GRAPH_BATCH", dflt);
	return b < 1 ? 1 : b;
}

}   // namespace

extern "C" yakamd_graph_t *yakamd_graph_open(yak_ch_t *h, int min_cnt)
{
	yakamd_ctx *c = yk_whole_image_ctx(h, min_cnt, "graph", "the graph has no CPU fallback",
	                                   "an even k-mer can be its own reverse complement, and a side's edges would not be distinct");
	if (!c) return 0;
	yakamd_graph_t *g = new (std::nothrow) yakamd_graph_t();
	if (!g) { fail("graph: no memory"); return 0; }
	g->h = h; g->c = c; g->min_cnt = min_cnt;
	g->keys_then = c->d_keys; g->slots_then = c->n_slots; g->total_then = c->img_keys_total;
	if (gr_build(g) != 0) { delete g; return 0; }
	return g;
}

extern "C" void yakamd_graph_close(yakamd_graph_t *g)
{
	if (!g) return;
	delete g;
}

extern "C" int yakamd_graph_stats(yakamd_graph_t *g, yakamd_gstat_t *st)
{
	if (gr_still(g, "graph stats")) return -1;
	if (!st) return fail("graph stats: no place for them");
	*st = g->st;
	return 0;
}

/* test and measurement hook: the milliseconds of the three steps of the open (edges, rank directory, links); measured when YAKAMD_VERBOSE or the
 * switch YAKAMD_GRAPH_TIMED is set, zero otherwise */
extern "C" void yakamd_graph_open_ms(yakamd_graph_t *g, double ms[3])
{
	ms[0] = g ? g->ms_edges : 0; ms[1] = g ? g->ms_rank : 0; ms[2] = g ? g->ms_link : 0;
}

/* measurement hook: the milliseconds the last yakamd_unitigs call of the process spent on the graph, on the records' way to the host, on the host
 * walk and on the text */
extern "C" void yakamd_unitigs_ms(double ms[4]) { for (int i = 0; i < 4; ++i) ms[i] = g_unitigs_ms[i]; }

extern "C" int64_t yakamd_graph_nodes_dev(yakamd_graph_t *g, int sub_lo, int sub_hi, void *d_nodes, int64_t cap)
{
	if (gr_still(g, "graph nodes")) return -1;
	yakamd_ctx *c = g->c;
	if (sub_lo < 0 || sub_hi < sub_lo || sub_hi > c->P) return fail("graph nodes: sub-tables [%d, %d) of %d", sub_lo, sub_hi, c->P);
	const u64 n = g->key0[sub_hi] - g->key0[sub_lo];
	if (!d_nodes || cap < (int64_t)n) return (int64_t)n;
	if (((uintptr_t)d_nodes & 15) != 0) return fail("graph nodes: the records must be 16-byte aligned");
	if (n == 0) return 0;
	HIPCK(hipSetDevice(c->dev));
	if (gr_launch(g, 3, g->tile0[sub_lo], g->tile0[sub_hi], d_nodes, g->key0[sub_lo], n)) return fail("graph nodes: the record kernel did not launch");
	HIPCK(hipStreamSynchronize(c->st));
	return (int64_t)n;
}

extern "C" void yakamd_ugopt_init(yakamd_ugopt_t *o)
{
	memset(o, 0, sizeof(yakamd_ugopt_t));
	o->min_cnt = 1;
	o->stats_only = 0;
	o->n_threads = 8;
	o->batch_keys = GR_BATCH_DEFAULT;
}

/* the command: the graph, its records to the host range by range, the walk, the text */
extern "C" int yakamd_unitigs(const yakamd_ugopt_t *opt, const yak_ch_t *ch, const char *out_fn)
{
	const double t_open = now_ms();
	struct Graph { yakamd_graph_t *g; ~Graph() { yakamd_graph_close(g); } } G{ yakamd_graph_open((yak_ch_t*)ch, opt->min_cnt) };
	yakamd_graph_t *g = G.g;
	if (!g) return -1;
	yakamd_ctx *c = g->c;
	const int k = ch->k, P = c->P;
	const u64 n_key = g->st.n_key;
	const double t0 = now_ms();
	std::vector<ug_node_t> nodes;
	try { nodes.resize((size_t)n_key); }
	catch (const std::bad_alloc&) { return fail("yakamd_unitigs: the records of %llu stored keys do not fit the host's memory (32 bytes each)", (unsigned long long)n_key); }
	const int64_t batch = gr_batch(opt->batch_keys);
	GrowBuf d_rec;
	const std::vector<TableRange> ranges = yk_ctx_ranges(c, 0, P, batch, false);   /* (those that hold keys) */
	for (const TableRange &r : ranges) {
		const u64 n = r.n();
		if (!d_rec.fit(n * sizeof(ug_node_t))) return fail("yakamd_unitigs: no device memory for %llu records", (unsigned long long)n);
		if (yakamd_graph_nodes_dev(g, r.lo, r.hi, d_rec.p, (int64_t)n) != (int64_t)n) return -1;
		if (yakamd_memcpy_d2h(nodes.data() + g->key0[r.lo], d_rec.p, n * sizeof(ug_node_t)) != 0) return -1;
	}
	d_rec.drop();
	const double t1 = now_ms();
	ug_result_t res;
	std::string err;
	try {
		if (ug_walk(nodes.data(), n_key, k, (uint32_t)opt->min_cnt, opt->n_threads, &res, &err) != 0) return fail("yakamd_unitigs: %s", err.c_str());
	} catch (const std::bad_alloc&) { return fail("yakamd_unitigs: the unitigs of %llu stored keys do not fit the host's memory", (unsigned long long)n_key); }
	const double t2 = now_ms();
	OutFile of;
	if (!of.open(out_fn)) return fail("yakamd_unitigs: cannot write '%s'", out_fn);
	FILE *out = of.f;
	bool ok = true;
	if (opt->stats_only) {
		const yakamd_gstat_t &s = g->st;
		fprintf(out, "#unitigs\tk=%d\tmin_cnt=%d\n", k, opt->min_cnt);
		fprintf(out, "N\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)s.n_key, (unsigned long long)s.n_node, (unsigned long long)s.n_arc, (unsigned long long)s.n_linked_side);
		for (int l = 0; l < 5; ++l)
			for (int r = 0; r < 5; ++r)
				if (s.deg[l][r]) fprintf(out, "D\t%d\t%d\t%llu\n", l, r, (unsigned long long)s.deg[l][r]);
		fputs(ug_stat_line(res).c_str(), out);
	} else ok = ug_fasta(res, [out](const std::string &t) { return fwrite(t.data(), 1, t.size(), out) == t.size(); });
	if (!of.finish() || !ok) return fail("yakamd_unitigs: cannot write '%s'", of.name);
	g_unitigs_ms[0] = t0 - t_open; g_unitigs_ms[1] = t1 - t0; g_unitigs_ms[2] = t2 - t1; g_unitigs_ms[3] = now_ms() - t2;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] unitigs: %zu ranges of records in %.1f ms, the host walk %.1f ms, the text %.1f ms\n", ranges.size(), t1 - t0, t2 - t1, now_ms() - t2);
	return 0;
}
