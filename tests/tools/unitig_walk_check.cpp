/* unitig_walk_check.cpp -- the host walk of `yak-amd unitigs` (yak_amd/csrc/unitig_walk.h) as a program of its own, for the host compiler and its
 * sanitizers: unitig_walk_check <records> <threads> fasta|stats reads the file tests/graph_util.py record_file() writes (k, min_cnt, the number
 * of records, the 32-byte records), walks it and prints the command's FASTA, or the U line of its -s form.  Exit 1 after a message when the file
 * cannot be read or the walk reports broken links. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../yak_amd/csrc/unitig_walk.h"

int main(int argc, char **argv)
{
	if (argc != 4) { fprintf(stderr, "usage: unitig_walk_check <records> <threads> fasta|stats\n"); return 2; }
	FILE *fp = fopen(argv[1], "rb");
	uint32_t head[2];
	uint64_t n = 0;
	if (!fp || fread(head, 4, 2, fp) != 2 || fread(&n, 8, 1, fp) != 1) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
	std::vector<ug_node_t> nd((size_t)n);
	if (n && fread(nd.data(), sizeof(ug_node_t), (size_t)n, fp) != n) { fprintf(stderr, "%s is short\n", argv[1]); return 1; }
	fclose(fp);
	ug_result_t res;
	std::string err;
	if (ug_walk(nd.data(), n, (int)head[0], head[1], atoi(argv[2]), &res, &err) != 0) { fprintf(stderr, "walk: %s\n", err.c_str()); return 1; }
	if (strcmp(argv[3], "stats") == 0) fputs(ug_stat_line(res).c_str(), stdout);
	else if (!ug_fasta(res, [](const std::string &t) { return fwrite(t.data(), 1, t.size(), stdout) == t.size(); })) return 1;
	return fflush(stdout) == 0 ? 0 : 1;
}
