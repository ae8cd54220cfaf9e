/* correct_text.h -- the two texts of `yak-amd correct` (include/yak_amd_correct.h) made on the host, HIP-free like
 * correct_step.h: the report's first line, an S line per sequence, an X line per fixed base, the T line, and a read in its normal form.  correct.hip
 * and tools/correct_model_check.cpp share it. */
#ifndef YK_CORRECT_TEXT_H
#define YK_CORRECT_TEXT_H
#include <stdio.h>
#include <string>
#include "correct_step.h"

struct crt_total_t { uint64_t n_seq, sum_len, v[7]; };

static inline void crt_decimal(std::string &text, uint64_t v)
{
	char buf[20];
	int n = 20;
	do { buf[--n] = (char)('0' + v % 10); v /= 10; } while (v);
	text.append(buf + n, (size_t)(20 - n));
}

/* `#correct k=<k> min_cnt=<c> min_run=<e>` */
static inline void crt_head(std::string &text, int k, int min_cnt, int min_run)
{
	char line[96];
	text.append(line, (size_t)snprintf(line, sizeof line, "#correct\tk=%d\tmin_cnt=%d\tmin_run=%d\n", k, min_cnt, min_run));
}

/* `S name len n_kmer n_weak n_cand n_fixed n_ambig n_nofit n_weak_after`, and the sequence into the sums */
static inline void crt_seq(std::string &text, const std::string &name, uint64_t len, const cr_tally_t &t, crt_total_t *tot)
{
	const uint32_t v[7] = { t.n_kmer, t.n_weak, t.n_cand, t.n_fixed, t.n_ambig, t.n_nofit, t.n_weak_after };
	text += "S\t"; text += name;
	text += '\t'; crt_decimal(text, len);
	for (int i = 0; i < 7; ++i) { text += '\t'; crt_decimal(text, v[i]); tot->v[i] += v[i]; }
	text += '\n';
	++tot->n_seq; tot->sum_len += len;
}

/* `X name p from to run_len` for a fixed record */
static inline void crt_fix(std::string &text, const std::string &name, const cr_fix_t &r)
{
	text += "X\t"; text += name;
	text += '\t'; crt_decimal(text, r.p);
	text += '\t'; text += (char)r.from;
	text += '\t'; text += (char)r.to;
	text += '\t'; crt_decimal(text, r.en - r.st);
	text += '\n';
}

/* `T n_seq sum_len` and the seven sums */
static inline void crt_last(std::string &text, const crt_total_t &tot)
{
	text += "T\t"; crt_decimal(text, tot.n_seq);
	text += '\t'; crt_decimal(text, tot.sum_len);
	for (int i = 0; i < 7; ++i) { text += '\t'; crt_decimal(text, tot.v[i]); }
	text += '\n';
}

/* a record in its normal form with `seq` (len bytes) for its sequence: `>name[ comment]\nSEQ\n`, or `@name[ comment]\nSEQ\n+\nQUAL\n` with a quality */
static inline void crt_read(std::string &text, const std::string &name, const std::string &comment, const std::string &qual, const char *seq, size_t len)
{
	text += qual.empty() ? '>' : '@';
	text += name;
	if (!comment.empty()) { text += ' '; text += comment; }
	text += '\n';
	text.append(seq, len);
	text += '\n';
	if (!qual.empty()) { text += "+\n"; text += qual; text += '\n'; }
}
#endif
