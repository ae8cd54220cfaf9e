/* hpc_host_check.cpp -- yk_hpc_host() and yk_hpc_back() (yak_amd/csrc/hpc_host.h: the host restatement of the homopolymer compression, which
 * yakamd_hpc_host() exports) on planted inputs, as a program of its own so that the host code can run under the sanitizers on the CPU:
 *     g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/tools/hpc_host_check.cpp -o /tmp/hpc_host_check && /tmp/hpc_host_check
 * Every output buffer is allocated at exactly the size the contract promises (n rounded up to 16), so a byte written beyond it is a report.
 * Prints "ok" and returns 0 when every case gives the expected bytes. */
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../yak_amd/csrc/hpc_host.h"

static unsigned char nt4[256];

static int check(const std::string &in, const std::string &want)
{
	std::vector<uint8_t> a(in.begin(), in.end());              /* exact sizes: the sanitizer sees the first byte beyond either */
	std::vector<uint8_t> out((in.size() + 15) / 16 * 16);
	const int64_t n = yk_hpc_host(nt4, a.data(), (int64_t)a.size(), out.data());
	std::string got((const char*)out.data(), (size_t)n);
	bool ok = got == want;
	for (size_t i = (size_t)n; i < ((size_t)n + 15) / 16 * 16; ++i) ok = ok && out[i] == '\n';
	if (!ok) fprintf(stderr, "FAILED on an input of %zu bytes: kept %ld, expected %zu\n", in.size(), (long)n, want.size());
	return ok ? 0 : 1;
}

int main(void)
{
	memset(nt4, 4, sizeof nt4);
	for (int i = 0; i < 4; ++i) nt4[i] = nt4[(unsigned char)"ACGT"[i]] = nt4[(unsigned char)"acgt"[i]] = (unsigned char)i;
	nt4['U'] = nt4['u'] = 3;
	int bad = 0;
	bad += check("", "");
	bad += check("A", "A");
	bad += check("AAAAAAA\n", "A\n");
	bad += check("AANAA\n", "A\nA\n");
	bad += check("Aa\nTU\ntuTU\n", "A\nT\nT\n");
	bad += check("AAACCCGTTNNAAT\n", "ACGT\n\nAT\n");
	bad += check("NNNN\n\n\n", "\n\n\n\n\n\n\n");
	bad += check(std::string("\0\0\1\1\2\3\3\n", 8), "ACGT\n");
	bad += check("ACGTTTT", "ACGT");                           /* a sequence that ends at the image's last byte */
	bad += check(std::string(70001, 'A') + "C\n", "AC\n");
	for (int n = 14; n <= 18; ++n) bad += check(std::string((size_t)n, 'G') + "T", "GT");
	{
		std::string alt, half;
		for (int i = 0; i < 4097; ++i) { alt += "ACGT"[i & 3]; alt += "ACGT"[i & 3]; half += "ACGT"[i & 3]; }
		bad += check(alt, half);
	}
	{	/* where a compressed stream may be cut: the chunk that continues AAACCGGGT| must open with its last two kept positions, the G run and T */
		const uint8_t s[] = "AAACCGGGT";
		if (yk_hpc_back(nt4, s, 9, 2) != 5 || yk_hpc_back(nt4, s, 9, 4) != 0 || yk_hpc_back(nt4, s, 9, 5) != -1 || yk_hpc_back(nt4, s, 9, 0) != 9 || yk_hpc_back(nt4, s, 8, 1) != 5) { fprintf(stderr, "FAILED: yk_hpc_back\n"); ++bad; }
	}
	if (bad) return 1;
	puts("ok");
	return 0;
}
