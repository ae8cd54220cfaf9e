/*
 * yak_qv_solve.cpp -- the host arithmetic of `yak qv` (reference qv.c:146-244): yak_qv_solve() and the solver it fits its parabola with.  No device
 * and no library state: two histograms in, the statistics out.
 */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/yak.h"

/* n x n linear system a x = b by Gauss-Jordan elimination with full pivoting (the solver the
 * reference links as 6gjdn.c); the solution replaces b.  false if the matrix is singular. */
static bool solve_full_pivot(double *a, double *b, int n)
{
	std::vector<int> col_of(n);
	for (int k = 0; k < n; ++k) {
		int pr = k, pc = k;
		double big = 0.0;
		for (int i = k; i < n; ++i)
			for (int j = k; j < n; ++j)
				if (fabs(a[i * n + j]) > big) { big = fabs(a[i * n + j]); pr = i; pc = j; }
		if (big + 1.0 == 1.0) return false;
		col_of[k] = pc;
		if (pc != k) for (int i = 0; i < n; ++i) std::swap(a[i * n + k], a[i * n + pc]);
		if (pr != k) { for (int j = k; j < n; ++j) std::swap(a[k * n + j], a[pr * n + j]); std::swap(b[k], b[pr]); }
		const double piv = a[k * n + k];
		for (int j = k + 1; j < n; ++j) a[k * n + j] /= piv;
		b[k] /= piv;
		for (int j = k + 1; j < n; ++j)
			for (int i = 0; i < n; ++i)
				if (i != k) a[i * n + j] -= a[i * n + k] * a[k * n + j];
		for (int i = 0; i < n; ++i)
			if (i != k) b[i] -= a[i * n + k] * b[k];
	}
	for (int k = n - 1; k >= 0; --k)                          /* undo the column exchanges */
		if (col_of[k] != k) std::swap(b[k], b[col_of[k]]);
	return true;
}

/* yak_qv_solve (reference qv.c:146-244): host arithmetic on two 1024-bin histograms -- in_table[c] = stored k-mers
 * that occur c times in the short reads, in_seqs[c] = k-mers of the assembly found with count c.  The statistics are
 * the reference's (raw QV from the share of absent k-mers; coverage at the histogram peak; bounds on the false-positive
 * rate of "absent"; corrected counts between the trough and the peak; successive ratios fitted by a parabola and
 * extrapolated to count 0; adjusted QV) and the printed digits must equal the reference's, so every floating-point
 * expression keeps the reference's operand order and association (sums run over ascending k, powers are built by
 * repeated multiplication).  That is the only thing shared with qv.c: the stages below are this file's own cut. */
namespace {
struct QvShape { int peak = -1, trough = -1; };

/* the mode of in_seqs over counts [2, 1023) and the lowest point in front of it */
QvShape qv_shape(const int64_t *in_seqs)
{
	QvShape s;
	int32_t top = 0;
	for (int c = 2; c < YAK_N_COUNTS - 1; ++c) if (top < in_seqs[c]) { top = (int32_t)in_seqs[c]; s.peak = c; }
	int32_t low = top;
	for (int c = 2; c < s.peak; ++c) if (low > in_seqs[c]) { low = (int32_t)in_seqs[c]; s.trough = c; }
	return s;
}

/* brackets the false-positive rate from the counts below the peak and clamps the caller's estimate into them */
double qv_fpr_bounds(const int64_t *in_table, const int64_t *in_seqs, const QvShape &s, double fpr, yak_qstat_t *qs)
{
	qs->fpr_upper = 1.0;
	for (int c = 2; c < s.peak; ++c) {
		const double e = in_seqs[c] / (qs->cov * in_table[c]);
		if (qs->fpr_upper > e) qs->fpr_upper = e;
	}
	if (fpr > qs->fpr_upper) fpr = qs->fpr_upper * 0.5;
	qs->fpr_lower = 0.0;
	if (s.trough > 2 && in_table[2] > in_table[s.trough]) {
		const double e = (in_seqs[2] - in_seqs[s.trough]) / (qs->cov * (in_table[2] - in_table[s.trough]));
		if (qs->fpr_lower < e) qs->fpr_lower = e;
	}
	if (fpr < qs->fpr_lower) fpr = qs->fpr_lower;
	if (qs->fpr_lower >= qs->fpr_upper)
		fprintf(stderr, "Warning: the FPR upper bound is smaller than the lower bound. Trust the lower bound.\n");
	return fpr;
}

/* least-squares polynomial of degree DEG through (x[k], y[k]), k < n, by the normal equations: coef[i] multiplies x^i.
 * pw[m][k] = x[k]^m by repeated multiplication; entry (i, j) of the matrix is the sum over k of pw[i + j][k] */
template <int DEG>
bool fit_polynomial(const double *x, const double *y, int n, double *coef)
{
	std::vector<double> pw((size_t)(2 * DEG + 1) * n);
	for (int k = 0; k < n; ++k) {
		double t = 1.0;
		for (int m = 0; m <= 2 * DEG; ++m) { pw[(size_t)m * n + k] = t; t *= x[k]; }
	}
	double M[(DEG + 1) * (DEG + 1)];
	for (int i = 0; i <= DEG; ++i) {
		for (int j = 0; j <= i; ++j) {
			double acc = 0.0;
			for (int k = 0; k < n; ++k) acc += pw[(size_t)(i + j) * n + k];
			M[i * (DEG + 1) + j] = M[j * (DEG + 1) + i] = acc;
		}
		double acc = 0.0;
		for (int k = 0; k < n; ++k) acc += pw[(size_t)i * n + k] * y[k];
		coef[i] = acc;
	}
	return solve_full_pivot(M, coef, DEG + 1);
}

template <int DEG> double eval_polynomial(const double *coef, double at)
{
	double r = 0.0, t = 1.0;
	for (int i = 0; i <= DEG; ++i) { r += coef[i] * t; t *= at; }
	return r;
}
} // namespace

extern "C" int yak_qv_solve(const int64_t *in_table, const int64_t *in_seqs, int kmer, double fpr, yak_qstat_t *qs)
{
	constexpr int DEG = 2, MAX_FIT = 8;
	const double db_per_ln = 4.3429448190325175;             /* 10 / ln 10 */
	memset(qs, 0, sizeof(*qs));
	for (int c = 0; c < YAK_N_COUNTS; ++c) { qs->tot += in_seqs[c]; qs->adj_cnt[c] = (double)in_seqs[c]; }
	qs->err = (double)in_seqs[0];
	qs->qv = -1.0;
	qs->qv_raw = (qs->tot > 0 && qs->tot > in_seqs[0]) ? -db_per_ln * log(log((double)qs->tot / (qs->tot - in_seqs[0])) / kmer) : -1.0;

	const QvShape s = qv_shape(in_seqs);
	if (s.peak < 0) return -1;                               /* nothing beyond count 1 */
	qs->cov = (double)in_seqs[s.peak] / in_table[s.peak];
	fpr = qv_fpr_bounds(in_table, in_seqs, s, fpr, qs);

	const int n_fit = std::min(MAX_FIT, s.peak - s.trough + 1);
	if (s.peak <= 4 || n_fit < 3) return -1;                 /* not high-coverage data: no adjustment */

	for (int c = s.peak - 1; c >= s.trough; --c) {           /* take the expected false "present" calls out */
		const double wrong = (in_table[c] - in_seqs[c] / qs->cov) / (1.0 - fpr);
		qs->adj_cnt[c] = in_seqs[c] - wrong * qs->cov * fpr;
		if (qs->adj_cnt[c] < 0.0) qs->adj_cnt[c] = 0.0;
	}

	double at[MAX_FIT], ratio[MAX_FIT], coef[DEG + 1];
	for (int k = 0; k < n_fit; ++k) { at[k] = s.trough + k; ratio[k] = qs->adj_cnt[s.trough + k + 1] / qs->adj_cnt[s.trough + k]; }
	if (!fit_polynomial<DEG>(at, ratio, n_fit, coef)) fprintf(stderr, "ERROR: fail\n");
	for (int c = s.trough - 1; c >= 0; --c) {                /* below the trough: divide down by the fitted ratio, at least 1.01 */
		double r = eval_polynomial<DEG>(coef, c);
		if (r < 1.01) r = 1.01;
		qs->adj_cnt[c] = qs->adj_cnt[c + 1] / r;
	}

	double adj_sum = 0.0;
	for (int c = 0; c < YAK_N_COUNTS; ++c) adj_sum += qs->adj_cnt[c];
	if (adj_sum <= (double)qs->tot) {
		qs->err = qs->tot - adj_sum;
		qs->qv = -db_per_ln * log(log(qs->tot / adj_sum) / kmer);
	} else {
		fprintf(stderr, "WARNING: failed to estimate the calibrated QV\n");
		qs->err = 0;
		qs->qv = qs->qv_raw;
	}
	return 0;
}
