// Differential splicing tests (step 4 of the pipeline, bin/Test_AS.r) on the device: Fisher's exact test per 2x2 table, the
// Poisson log-linear model + likelihood-ratio test per form, the Wilcoxon rank-sum test per form, and the Bonferroni / BH
// corrections (R's p.adjust); beside them this project's own replicate-aware test, a beta-binomial model with one dispersion per row.  FP64 throughout; NaN stands for R's NA.  The rules each kernel follows are spelled out in
// DESIGN.md ("Differential splicing tests"); the host side (readers, formatter, the test_as executable) is lsq_as.cpp.
//
//   lsq_as_fisher_kernel   one wave per table: the hypergeometric pmf walked outward from its mode, 64 terms a step
//   lsq_as_lrt_kernel      one lane per row: two IRLS fits (R's glm.fit), normal equations in registers, Cholesky; the difference of their deviances
//   lsq_as_betabin_kernel  one lane per row: per model a grid in rho and Brent's minimiser over a profile whose inner maxima in mu are safeguarded Newton
//                          solves; log-gamma and digamma differences as a few direct terms plus a difference of two Stirling forms
//   lsq_as_wilcox_kernel   one lane per row: W and the tie groups by counting over the row; exact tables from the host
//   correction             NA compaction (lsq_scan.hpp, flag mode), stable LSD radix sort of (p bits, index) (lsq_sort.hpp), reverse min-scan
#include <cfloat>

#include "lsq_device.hpp"
#include "lsq_scan.hpp"
#include "lsq_sort.hpp"

namespace {

constexpr double FISHER_REL_ERR = 1.0 + 1e-7;   // fisher.test's relErr
constexpr double LOG_FLOOR = -746.0;            // exp() of anything below is 0 in double
constexpr double AS_MAX_CELL = 1099511627776.0; // 2^40
constexpr int GLM_MAXIT = 25;                   // glm.control()
constexpr double GLM_EPS = 1e-8;
constexpr int WILCOX_EXACT_MAX = 50;            // wilcox.test: exact when both groups have fewer values, and no ties

__device__ inline double wave_incl_sum(double v) {
	const unsigned lane = threadIdx.x & 63u;
#pragma unroll
	for (unsigned d = 1; d < 64; d <<= 1) {
		const double o = __shfl_up(v, d);
		if (lane >= d) v += o;
	}
	return v;
}

__device__ inline double wave_sum(double v) {
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
	return v;
}

// ---- Fisher ---------------------------------------------------------------------------------------------------------

struct Hyper {
	long long m, n, k, lo, hi, mode;
	// log d(s+1)/d(s) for lo <= s < hi: one log per term (lgamma differences lose ~1e-8 at counts of 10^6)
	__device__ double step(long long s) const {
		return log(((double)(m - s) / (double)(s + 1)) * ((double)(k - s) / (double)(n - k + s + 1)));
	}
};

// floor((k+1)(m+1)/(m+n+2)) exactly: a double estimate, corrected with 128-bit products (no 128-bit division)
__device__ inline long long hyper_mode(long long m, long long n, long long k) {
	typedef unsigned __int128 u128;
	const unsigned long long a = (unsigned long long)(k + 1), b = (unsigned long long)(m + 1), N = (unsigned long long)(m + n + 2);
	const u128 P = (u128)a * b;
	long long q = (long long)floor(((double)a * (double)b) / (double)N);
	if (q < 0) q = 0;
	while ((u128)(unsigned long long)q * N > P) --q;
	while ((u128)(unsigned long long)(q + 1) * N <= P) ++q;
	return q;
}

// One wave per table (grid-stride over tables).  Every branch below is uniform over the wave.
__global__ void __launch_bounds__(256) lsq_as_fisher_kernel(const double *cells, unsigned long long n_tables, double *p_out) {
	const unsigned lane = threadIdx.x & 63u;
	const unsigned long long waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
	for (unsigned long long t = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n_tables; t += waves) {
		double c[4];
		bool na = false;
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			c[q] = rint(cells[t * 4 + q]);
			if (!(c[q] >= 0.0 && c[q] <= AS_MAX_CELL)) na = true;     // NA, negative, infinite or beyond 2^40
		}
		if (na) { if (lane == 0) p_out[t] = NAN; continue; }
		Hyper h;
		const long long A = (long long)c[0], B = (long long)c[1], C = (long long)c[2], D = (long long)c[3];
		h.m = A + B; h.n = C + D; h.k = A + C;
		const long long x = A;
		h.lo = h.k - h.n > 0 ? h.k - h.n : 0;
		h.hi = h.k < h.m ? h.k : h.m;
		h.mode = hyper_mode(h.m, h.n, h.k);
		if (h.mode < h.lo) h.mode = h.lo;
		if (h.mode > h.hi) h.mode = h.hi;
		if (h.lo == h.hi) { if (lane == 0) p_out[t] = 1.0; continue; }

		// log d(x)/d(mode), walking from the mode towards x; below LOG_FLOOR d(x) is 0, as in R, and so is p
		double Lx = 0.0;
		bool x_zero = false;
		if (x != h.mode) {
			const long long dir = x > h.mode ? 1 : -1, dist = x > h.mode ? x - h.mode : h.mode - x;
			double carry = 0.0;
			for (long long j0 = 0;; j0 += 64) {
				const long long j = j0 + lane + 1, s = h.mode + dir * j;
				const double term = j <= dist ? (dir > 0 ? h.step(s - 1) : -h.step(s)) : 0.0;
				const double L = carry + wave_incl_sum(term);
				if (dist <= j0 + 64) { Lx = __shfl(L, (int)(dist - j0 - 1)); break; }
				carry = __shfl(L, 63);
				if (__all(L < LOG_FLOOR)) { x_zero = true; break; }
			}
		}
		if (x_zero) { if (lane == 0) p_out[t] = 0.0; continue; }

		// both sums over the window around the mode where terms are non-zero (the pmf is log-concave: once a whole chunk
		// is below LOG_FLOOR every term further out is too)
		const double thr = exp(Lx) * FISHER_REL_ERR;
		double total = 0.0, num = 0.0;
		for (int side = 0; side < 2; ++side) {
			const long long dir = side == 0 ? 1 : -1, limit = side == 0 ? h.hi - h.mode : h.mode - h.lo;
			double carry = 0.0;
			for (long long j0 = 0; j0 < limit; j0 += 64) {
				const long long j = j0 + lane + 1, s = h.mode + dir * j;
				const bool valid = j <= limit;
				const double term = valid ? (dir > 0 ? h.step(s - 1) : -h.step(s)) : 0.0;
				const double L = carry + wave_incl_sum(term);
				const double e = valid ? exp(L) : 0.0;
				total += e;
				if (e <= thr) num += e;
				carry = __shfl(L, 63);
				if (__all(!valid || L < LOG_FLOOR)) break;
			}
		}
		total = 1.0 + wave_sum(total);
		num = (1.0 <= thr ? 1.0 : 0.0) + wave_sum(num);
		if (lane == 0) p_out[t] = num / total;
	}
}

// ---- Poisson log-linear model + LRT -----------------------------------------------------------------------------------

// Columns of a design: the intercept, then tissue (if TISSUE), then rep while columns remain.
template <int P, bool TISSUE>
__device__ inline void design_row(double tissue, double rep, double *x) {
	x[0] = 1.0;
	if (P >= 2) x[1] = TISSUE ? tissue : rep;
	if (P >= 3) x[2] = rep;
}

// A x = b for a symmetric positive definite P x P matrix in packed lower storage (a[i*(i+1)/2 + j], j <= i).
// false when a pivot is not positive.
template <int P>
__device__ inline bool cholesky_solve(const double *a, const double *b, double *x) {
	double l[P * (P + 1) / 2];
#pragma unroll
	for (int i = 0; i < P; ++i) {
#pragma unroll
		for (int j = 0; j <= i; ++j) {
			double s = a[i * (i + 1) / 2 + j];
#pragma unroll
			for (int q = 0; q < j; ++q) s -= l[i * (i + 1) / 2 + q] * l[j * (j + 1) / 2 + q];
			if (i == j) {
				if (!(s > 0.0)) return false;
				l[i * (i + 1) / 2 + i] = sqrt(s);
			} else {
				l[i * (i + 1) / 2 + j] = s / l[j * (j + 1) / 2 + j];
			}
		}
	}
	double y[P];
#pragma unroll
	for (int i = 0; i < P; ++i) {
		double s = b[i];
#pragma unroll
		for (int q = 0; q < i; ++q) s -= l[i * (i + 1) / 2 + q] * y[q];
		y[i] = s / l[i * (i + 1) / 2 + i];
	}
#pragma unroll
	for (int i = P - 1; i >= 0; --i) {
		double s = y[i];
#pragma unroll
		for (int q = i + 1; q < P; ++q) s -= l[q * (q + 1) / 2 + i] * x[q];
		x[i] = s / l[i * (i + 1) / 2 + i];
	}
	return true;
}

// One observation's share of the Poisson deviance, 2 (y log(y/mu) - (y - mu)), as 2 mu ((1 + r) log1p(r) - r) with
// r = (y - mu)/mu: the first form subtracts two numbers of the size of y (an error of 1e-4 at y = 10^12), the second
// works on r alone and keeps the share to a relative 1e-9 or better.  y >= 1 here, so r > -1.
__device__ inline double poisson_dev(double y, double mu) {
	const double r = (y - mu) / mu;
	return 2.0 * mu * ((1.0 + r) * log1p(r) - r);
}

// R's glm.fit for family = poisson(log) with an offset: start at mu = y + 0.1, WLS by the normal equations, stop on the
// relative deviance change or after GLM_MAXIT solves.  y and o lie sample-major (y[j * stride]).  Returns the deviance
// of the last iterate, NaN when a solve fails.
template <int P, bool TISSUE>
__device__ double glm_poisson(const double *y, const double *o, unsigned long long stride, int n1, int n) {
	double a[P * (P + 1) / 2], b[P], beta[P], x[P];
#pragma unroll
	for (int q = 0; q < P * (P + 1) / 2; ++q) a[q] = 0.0;
#pragma unroll
	for (int q = 0; q < P; ++q) b[q] = 0.0;
	double dev_old = 0.0, dev = 0.0;
	for (int j = 0; j < n; ++j) {
		const double yj = y[(unsigned long long)j * stride], oj = o[(unsigned long long)j * stride];
		const double eta = log(yj + 0.1), mu = fmax(exp(eta), DBL_EPSILON);
		dev_old += poisson_dev(yj, mu);
		design_row<P, TISSUE>(j < n1 ? 1.0 : 2.0, (double)(j < n1 ? j + 1 : j - n1 + 1), x);
		const double z = (eta - oj) + (yj - mu) / mu;
#pragma unroll
		for (int r = 0; r < P; ++r) {
			b[r] += mu * x[r] * z;
#pragma unroll
			for (int s = 0; s <= r; ++s) a[r * (r + 1) / 2 + s] += mu * x[r] * x[s];
		}
	}
	for (int it = 0; it < GLM_MAXIT; ++it) {
		if (!cholesky_solve<P>(a, b, beta)) return NAN;
		dev = 0.0;
#pragma unroll
		for (int q = 0; q < P * (P + 1) / 2; ++q) a[q] = 0.0;
#pragma unroll
		for (int q = 0; q < P; ++q) b[q] = 0.0;
		for (int j = 0; j < n; ++j) {
			const double yj = y[(unsigned long long)j * stride], oj = o[(unsigned long long)j * stride];
			design_row<P, TISSUE>(j < n1 ? 1.0 : 2.0, (double)(j < n1 ? j + 1 : j - n1 + 1), x);
			double lin = 0.0;
#pragma unroll
			for (int r = 0; r < P; ++r) lin += x[r] * beta[r];
			const double eta = lin + oj, mu = fmax(exp(eta), DBL_EPSILON);
			dev += poisson_dev(yj, mu);
			const double z = (eta - oj) + (yj - mu) / mu;
#pragma unroll
			for (int r = 0; r < P; ++r) {
				b[r] += mu * x[r] * z;
#pragma unroll
				for (int s = 0; s <= r; ++s) a[r * (r + 1) / 2 + s] += mu * x[r] * x[s];
			}
		}
		if (fabs(dev - dev_old) / (fabs(dev) + 0.1) < GLM_EPS) break;
		dev_old = dev;
	}
	return dev;
}

// One lane per row.  count / total arrive sample-major ([sample][row]) and are turned in place into y = round(count) + 1
// and the offset log(round(total) + 1) -- each lane rewrites its own column only.
__global__ void __launch_bounds__(256) lsq_as_lrt_kernel(double *count, double *total, unsigned long long n_rows, int n1, int n2,
                                                          double *stat_out, double *p_out) {
	const int n = n1 + n2;
	const bool aliased = n1 == 1 && n2 == 1;      // rep is constant: R drops it (ranks 2 and 1)
	for (unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (unsigned long long)gridDim.x * blockDim.x) {
		bool na = false;
		for (int j = 0; j < n; ++j) {
			const double c = rint(count[(unsigned long long)j * n_rows + r]), tt = rint(total[(unsigned long long)j * n_rows + r]);
			if (!(c >= 0.0 && c < INFINITY) || !(tt >= 0.0 && tt < INFINITY)) na = true;
			count[(unsigned long long)j * n_rows + r] = c + 1.0;
			total[(unsigned long long)j * n_rows + r] = log(tt + 1.0);
		}
		if (na) { stat_out[r] = NAN; p_out[r] = NAN; continue; }
		const double *y = count + r, *o = total + r;
		double df, dr;
		if (aliased) {
			df = glm_poisson<2, true>(y, o, n_rows, n1, n);
			dr = glm_poisson<1, false>(y, o, n_rows, n1, n);
		} else {
			df = glm_poisson<3, true>(y, o, n_rows, n1, n);
			dr = glm_poisson<2, false>(y, o, n_rows, n1, n);
		}
		// the difference of the two deviances is 2 (l_full - l_reduced) exactly; the log-likelihoods themselves are 10^10
		// times the statistic at totals of 10^8, and their difference kept five digits of it
		const double stat = fabs(dr - df);
		if (!isfinite(df) || !isfinite(dr) || isnan(stat)) { stat_out[r] = 0.0; p_out[r] = 1.0; continue; }   // Test_AS.r:112-114
		stat_out[r] = stat;
		p_out[r] = erfc(sqrt(stat / 2.0));      // upper chi-square tail, one degree of freedom
	}
}

// ---- beta-binomial model + LRT ------------------------------------------------------------------------------------------

// y_j ~ BetaBinomial(n_j, a, b), a = mu (1 - rho)/rho, b = (1 - mu)(1 - rho)/rho, the binomial coefficient dropped:
//   l_j(mu, rho) = E(mu (1 - rho), rho, y) + E((1 - mu)(1 - rho), rho, n - y) - E(1 - rho, rho, n),   E(c, rho, k) = sum_{i<k} ln(c + i rho).
// For rho > 0, E = k ln rho + L(c / rho, k) with L(x, k) = sum_{i<k} ln(x + i) = lgamma(x + k) - lgamma(x); the three k ln rho of a
// sample cancel (y + (n - y) - n = 0) and are never formed.  At rho = 0 the sample is binomial.
constexpr double BB_RHO_MAX = 0.999;
constexpr double BB_SHIFT_TO = 8.0;       // the Stirling series start at x >= 8: the first term left out of each is below 5e-13 there
constexpr int BB_GRID = 18;               // grid in rho: 0, then BB_GRID points, two a decade, the last BB_RHO_MAX (the first 3.2e-9)
constexpr int BB_NEWTON_MAXIT = 40;       // solves for one mu at one rho
constexpr int BB_BRENT_MAXIT = 48;        // profile evaluations after the grid
constexpr double BB_MU_TOL = 1e-6;        // Newton stops at a step below this times min(mu, 1 - mu): quadratic, so mu is then good to ~1e-12 of itself and l to ~1e-24 of the row's reads
constexpr double BB_RHO_RTOL = 1.5e-8;    // sqrt(DBL_EPSILON): closer than this two profile values do not differ
constexpr double BB_RHO_ATOL = 1e-5;      // times the bracket's width: what an optimum at rho = 0 is approached to

// lgamma(z) - ((z - 1/2) ln z - z + ln(2 pi)/2) as a series in w = 1/z (through B_12)
__device__ inline double bb_stirling(double w) {
	const double w2 = w * w;
	return w * (1.0 / 12.0 + w2 * (-1.0 / 360.0 + w2 * (1.0 / 1260.0 + w2 * (-1.0 / 1680.0 + w2 * (1.0 / 1188.0 + w2 * (-691.0 / 360360.0))))));
}
// ln z - digamma(z), w = 1/z (through B_10)
__device__ inline double bb_digamma_tail(double w) {
	const double w2 = w * w;
	return 0.5 * w + w2 * (1.0 / 12.0 + w2 * (-1.0 / 120.0 + w2 * (1.0 / 252.0 + w2 * (-1.0 / 240.0 + w2 * (1.0 / 132.0)))));
}
// trigamma(z) - 1/z, w = 1/z (through B_10)
__device__ inline double bb_trigamma_tail(double w) {
	const double w2 = w * w;
	return w2 * (0.5 + w * (1.0 / 6.0 + w2 * (-1.0 / 30.0 + w2 * (1.0 / 42.0 + w2 * (-1.0 / 30.0 + w2 * (5.0 / 66.0))))));
}

// the terms taken directly before the series: enough to lift x to BB_SHIFT_TO, at most 8 and at most k
__device__ inline double bb_shift(double x, double k) {
	const double m = x >= BB_SHIFT_TO ? 0.0 : ceil(BB_SHIFT_TO - x);
	return fmin(m, k);
}

// L(x, k) = sum_{i<k} ln(x + i), x >= 0, k a whole number: m direct terms (their product, one log; ln 0 = -inf at x = 0), then with
// z = x + m and q = k - m the difference of two Stirling forms, (z - 1/2) log1p(q/z) + q ln(z + q) - q + S(z + q) - S(z).  A bounded
// number of operations whatever k is; k <= m leaves q = 0 and the direct terms alone.
__device__ inline double bb_logsum(double x, double k) {
	if (!(k > 0.0)) return 0.0;
	const double m = bb_shift(x, k), z = x + m, q = k - m;
	double g = 0.0;
	if (m > 0.0) {
		double prod = 1.0;
		for (double i = 0.0; i < m; i += 1.0) prod *= x + i;
		g = log(prod);
	}
	if (q > 0.0) {
		const double zq = z + q;
		g += (z - 0.5) * log1p(q / z) + q * log(zq) - q + (bb_stirling(1.0 / zq) - bb_stirling(1.0 / z));
	}
	return g;
}

// The same shape for the derivatives the Newton step needs: d = sum_{i<k} 1/(x + i) = digamma(x + k) - digamma(x) and
// t = sum_{i<k} 1/(x + i)^2 = trigamma(x) - trigamma(x + k).  The leading term of t is q/(z (z + q)), not 1/z - 1/(z + q).
__device__ inline void bb_dsum(double x, double k, double &d, double &t) {
	d = 0.0; t = 0.0;
	if (!(k > 0.0)) return;
	const double m = bb_shift(x, k), z = x + m, q = k - m;
	for (double i = 0.0; i < m; i += 1.0) { const double r = 1.0 / (x + i); d += r; t += r * r; }
	if (q > 0.0) {
		const double w0 = 1.0 / z, w1 = 1.0 / (z + q);
		d += log1p(q * w0) - (bb_digamma_tail(w1) - bb_digamma_tail(w0));
		t += q * w0 * w1 + (bb_trigamma_tail(w0) - bb_trigamma_tail(w1));
	}
}

__device__ inline double bb_xlogy(double x, double y) { return x == 0.0 ? 0.0 : x * log(y); }     // 0 ln 0 = 0

// sum over the samples j0 <= j < j1 of l_j(mu, rho); y and n lie sample-major (y[j * stride]).  -inf where a sample has y > 0 at mu = 0
// or y < n at mu = 1.  The fit and lsq_debug_as_bb_loglik both call this.
__device__ double bb_loglik(const double *y, const double *n, unsigned long long stride, int j0, int j1, double mu, double rho) {
	if (rho == 0.0) {
		double sy = 0.0, sm = 0.0;
		for (int j = j0; j < j1; ++j) { const double yj = y[(unsigned long long)j * stride]; sy += yj; sm += n[(unsigned long long)j * stride] - yj; }
		return bb_xlogy(sy, mu) + bb_xlogy(sm, 1.0 - mu);
	}
	const double s = (1.0 - rho) / rho, a = mu * s, b = (1.0 - mu) * s;
	double l = 0.0;
	for (int j = j0; j < j1; ++j) {
		const double yj = y[(unsigned long long)j * stride], nj = n[(unsigned long long)j * stride];
		l += (bb_logsum(a, yj) + bb_logsum(b, nj - yj)) - bb_logsum(s, nj);
	}
	return l;
}

// One row of the fit: its samples, and per condition the sums of y and of n - y.
struct BbRow {
	const double *y, *n;
	unsigned long long stride;
	int n1, n_all;
	double sy[2], sm[2];
};

// argmax over mu in [0, 1] of the samples j0 <= j < j1 at one rho > 0 (s = (1 - rho)/rho), from the start `mu` in (0, 1).  l is
// concave in mu, so its derivative s sum(d_a - d_b) falls: Newton on it inside a bracket that each evaluation tightens, the
// midpoint where a step leaves the bracket or is no number.  No y at all puts the maximum at mu = 0, no n - y at mu = 1.
__device__ double bb_solve_mu(const BbRow &r, int j0, int j1, double sy, double sm, double s, double mu) {
	if (sy == 0.0) return 0.0;
	if (sm == 0.0) return 1.0;
	double lo = 0.0, hi = 1.0;
	for (int it = 0; it < BB_NEWTON_MAXIT; ++it) {
		const double a = mu * s, b = (1.0 - mu) * s;
		double g = 0.0, h = 0.0;
		for (int j = j0; j < j1; ++j) {
			const double yj = r.y[(unsigned long long)j * r.stride], nj = r.n[(unsigned long long)j * r.stride];
			double d, t;
			bb_dsum(a, yj, d, t); g += d; h += t;
			bb_dsum(b, nj - yj, d, t); g -= d; h += t;
		}
		if (g > 0.0) lo = mu; else if (g < 0.0) hi = mu; else break;
		double next = mu + g / (s * h);
		if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
		const double step = fabs(next - mu);
		mu = next;
		if (step <= BB_MU_TOL * fmin(mu, 1.0 - mu)) break;
	}
	return mu;
}

// max over the mu of l at one rho, and where: FULL one mu per condition (they separate), else one for all samples (in mu1).
// mu1 / mu2 come in as the starts (the maxima at a rho nearby).
template <bool FULL>
__device__ double bb_profile(const BbRow &r, double rho, double &mu1, double &mu2) {
	const double sy = r.sy[0] + r.sy[1], sm = r.sm[0] + r.sm[1];
	if (rho == 0.0) {
		if (FULL) {
			mu1 = r.sy[0] / (r.sy[0] + r.sm[0]); mu2 = r.sy[1] / (r.sy[1] + r.sm[1]);
			return (bb_xlogy(r.sy[0], mu1) + bb_xlogy(r.sm[0], 1.0 - mu1)) + (bb_xlogy(r.sy[1], mu2) + bb_xlogy(r.sm[1], 1.0 - mu2));
		}
		mu1 = sy / (sy + sm);
		return bb_xlogy(sy, mu1) + bb_xlogy(sm, 1.0 - mu1);
	}
	const double s = (1.0 - rho) / rho;
	if (FULL) {
		mu1 = bb_solve_mu(r, 0, r.n1, r.sy[0], r.sm[0], s, mu1);
		mu2 = bb_solve_mu(r, r.n1, r.n_all, r.sy[1], r.sm[1], s, mu2);
		return bb_loglik(r.y, r.n, r.stride, 0, r.n1, mu1, rho) + bb_loglik(r.y, r.n, r.stride, r.n1, r.n_all, mu2, rho);
	}
	mu1 = bb_solve_mu(r, 0, r.n_all, sy, sm, s, mu1);
	return bb_loglik(r.y, r.n, r.stride, 0, r.n_all, mu1, rho);
}

// dl/drho at rho = 0 of the samples j0 <= j < j1 (d/drho ln(c (1 - rho) + i rho) = (i - c)/c there), at their binomial maximum mu: the
// slope of the profile at its left end, since there the mu-derivative is 0, or mu sits at 0 or 1 and the samples' terms are 0.
__device__ double bb_slope_at_zero(const BbRow &r, int j0, int j1, double mu) {
	double s = 0.0;
	for (int j = j0; j < j1; ++j) {
		const double yj = r.y[(unsigned long long)j * r.stride], nj = r.n[(unsigned long long)j * r.stride], mj = nj - yj;
		double t = nj - 0.5 * nj * (nj - 1.0);
		if (yj > 0.0) t += (0.5 * yj * (yj - 1.0) - yj * mu) / mu;
		if (mj > 0.0) t += (0.5 * mj * (mj - 1.0) - mj * (1.0 - mu)) / (1.0 - mu);
		s += t;
	}
	return s;
}

__device__ inline double bb_grid_rho(int i) {      // 0, then two a decade up to BB_RHO_MAX
	return i == 0 ? 0.0 : BB_RHO_MAX * exp(-1.151292546497023 * (double)(BB_GRID - i));     // ln(10)/2
}

// The maximum of the profile over rho in [0, BB_RHO_MAX]: the grid, then Brent's minimiser (parabolic steps, golden-section
// steps where those fail) on -profile between the two neighbours of the grid's best point, started at that point.  Every loop
// is capped; the best point evaluated is what comes back, the grid's own points included, so a maximum at either end of the
// domain is returned exactly.  The profile is not proved unimodal: between the neighbours of the best grid
// point this finds a local maximum no lower than that point.
template <bool FULL>
__device__ void bb_fit(const BbRow &r, double &l_out, double &rho_out, double &mu1_out, double &mu2_out) {
	double mu1 = 0.5, mu2 = 0.5;
	double fx = INFINITY, x = 0.0, xm1 = 0.5, xm2 = 0.5;      // f = -profile
	int ib = 0;
	for (int i = 0; i <= BB_GRID; ++i) {
		const double rho = bb_grid_rho(i), f = -bb_profile<FULL>(r, rho, mu1, mu2);
		if (f < fx) { fx = f; x = rho; xm1 = mu1; xm2 = mu2; ib = i; }
	}
	if (ib == 0) {
		// the binomial fit is the grid's best and the profile falls away from it: replicates that agree as well as binomial draws,
		// the commonest row there is.  rho = 0 is then a local maximum, and the search that would only close in on it is left out.
		const double slope = FULL ? bb_slope_at_zero(r, 0, r.n1, xm1) + bb_slope_at_zero(r, r.n1, r.n_all, xm2) : bb_slope_at_zero(r, 0, r.n_all, xm1);
		if (slope <= 0.0) { l_out = -fx; rho_out = 0.0; mu1_out = xm1; mu2_out = xm2; return; }
	}
	double a = bb_grid_rho(ib > 0 ? ib - 1 : 0), b = bb_grid_rho(ib < BB_GRID ? ib + 1 : BB_GRID);
	const double atol = BB_RHO_ATOL * (b - a);
	double w = x, v = x, fw = fx, fv = fx, d = 0.0, e = 0.0;
	for (int it = 0; it < BB_BRENT_MAXIT; ++it) {
		const double mid = 0.5 * (a + b), tol1 = BB_RHO_RTOL * fabs(x) + atol, tol2 = 2.0 * tol1;
		if (fabs(x - mid) <= tol2 - 0.5 * (b - a)) break;
		bool golden = true;
		if (fabs(e) > tol1) {
			const double rr = (x - w) * (fx - fv);
			double q = (x - v) * (fx - fw), p = (x - v) * q - (x - w) * rr;
			q = 2.0 * (q - rr);
			if (q > 0.0) p = -p;
			q = fabs(q);
			const double e_old = e;
			e = d;
			if (fabs(p) < fabs(0.5 * q * e_old) && p > q * (a - x) && p < q * (b - x)) {
				d = p / q;
				const double u = x + d;
				if (u - a < tol2 || b - u < tol2) d = copysign(tol1, mid - x);
				golden = false;
			}
		}
		if (golden) { e = x >= mid ? a - x : b - x; d = 0.3819660112501051 * e; }
		const double u = fabs(d) >= tol1 ? x + d : x + copysign(tol1, d);
		mu1 = xm1; mu2 = xm2;
		const double fu = -bb_profile<FULL>(r, u, mu1, mu2);
		if (fu <= fx) {
			if (u >= x) a = x; else b = x;
			v = w; fv = fw; w = x; fw = fx; x = u; fx = fu; xm1 = mu1; xm2 = mu2;
		} else {
			if (u < x) a = u; else b = u;
			if (fu <= fw || w == x) { v = w; fv = fw; w = u; fw = fu; }
			else if (fu <= fv || v == x || v == w) { v = u; fv = fu; }
		}
	}
	l_out = -fx; rho_out = x; mu1_out = xm1; mu2_out = xm2;
}

// One lane per row (DESIGN.md 4.6 says why).  count / total arrive sample-major and are rounded in place to y and n -- each
// lane rewrites its own column only.  A sample with n = 0 adds nothing to any sum, so it needs no skipping, only counting.
__global__ void __launch_bounds__(64) lsq_as_betabin_kernel(double *count, double *total, unsigned long long n_rows, int n1, int n2,
                                                              double *mu1_out, double *mu2_out, double *rho_out, double *stat_out, double *p_out) {
	const int n = n1 + n2;
	for (unsigned long long row = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (unsigned long long)gridDim.x * blockDim.x) {
		BbRow r;
		r.y = count + row; r.n = total + row; r.stride = n_rows; r.n1 = n1; r.n_all = n;
		bool na = false;
		int inf1 = 0, inf2 = 0;                   // informative samples (n > 0) per condition
		double sy1 = 0.0, sm1 = 0.0, sy2 = 0.0, sm2 = 0.0;
		for (int j = 0; j < n; ++j) {
			const double c = rint(count[(unsigned long long)j * n_rows + row]), tt = rint(total[(unsigned long long)j * n_rows + row]);
			if (!(c >= 0.0 && c <= AS_MAX_CELL) || !(tt >= 0.0 && tt <= AS_MAX_CELL) || c > tt) na = true;
			count[(unsigned long long)j * n_rows + row] = c;
			total[(unsigned long long)j * n_rows + row] = tt;
			if (j < n1) { inf1 += tt > 0.0; sy1 += c; sm1 += tt - c; }
			else { inf2 += tt > 0.0; sy2 += c; sm2 += tt - c; }
		}
		r.sy[0] = sy1; r.sy[1] = sy2; r.sm[0] = sm1; r.sm[1] = sm2;
		double mu1 = NAN, mu2 = NAN, rho = NAN, stat = NAN, p = NAN;
		if (!na && inf1 > 0 && inf2 > 0 && inf1 + inf2 >= 3) {
			if (r.sy[0] + r.sy[1] == 0.0 || r.sm[0] + r.sm[1] == 0.0) {
				// all y = 0 or all y = n: both profiles are 0 at every rho, the maximum is attained on the whole interval
				mu1 = mu2 = r.sy[0] + r.sy[1] == 0.0 ? 0.0 : 1.0; rho = 0.0; stat = 0.0; p = 1.0;
			} else {
				double lf, lr, rho_r, m1_r, m2_r;
				bb_fit<true>(r, lf, rho, mu1, mu2);
				bb_fit<false>(r, lr, rho_r, m1_r, m2_r);
				stat = fmax(0.0, 2.0 * (lf - lr));
				p = erfc(sqrt(stat / 2.0));      // upper chi-square tail, one degree of freedom
			}
		}
		mu1_out[row] = mu1; mu2_out[row] = mu2; rho_out[row] = rho; stat_out[row] = stat; p_out[row] = p;
	}
}

// lsq_debug_as_bb_loglik: one lane per row, y and n sample-major as the fit reads them
__global__ void __launch_bounds__(256) lsq_as_bb_loglik_kernel(const double *y, const double *n, unsigned long long n_rows, int n_samples,
                                                                const double *mu, const double *rho, double *out) {
	for (unsigned long long row = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (unsigned long long)gridDim.x * blockDim.x)
		out[row] = bb_loglik(y + row, n + row, n_rows, 0, n_samples, mu[row], rho[row]);
}

// ---- Wilcoxon rank-sum --------------------------------------------------------------------------------------------------

// mean() of R: the sum over n, then the mean of the residuals added (in double here; R sums in long double)
__device__ inline double r_mean(const double *v, unsigned long long stride, int first, int cnt) {
	double s = 0.0;
	for (int j = first; j < first + cnt; ++j) s += v[(unsigned long long)j * stride];
	s /= cnt;
	if (isfinite(s)) {
		double t = 0.0;
		for (int j = first; j < first + cnt; ++j) t += v[(unsigned long long)j * stride] - s;
		s += t / cnt;
	}
	return s;
}

// One lane per row, values sample-major.  exact_off[nx * WILCOX_EXACT_MAX + ny]: where the lower CDF of W for (nx, ny)
// starts in exact_cdf (nx*ny + 1 values), -1 when the host built none.
__global__ void __launch_bounds__(256) lsq_as_wilcox_kernel(const double *value, unsigned long long n_rows, int n1, int n2,
                                                             const long long *exact_off, const double *exact_cdf,
                                                             double *diff_out, double *p_out) {
	const int n = n1 + n2;
	for (unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (unsigned long long)gridDim.x * blockDim.x) {
		const double *v = value + r;
		bool any_nan = false;
		int nx = 0, ny = 0;
		for (int j = 0; j < n; ++j) {
			const double a = v[(unsigned long long)j * n_rows];
			any_nan |= isnan(a);
			if (isfinite(a)) { if (j < n1) ++nx; else ++ny; }
		}
		diff_out[r] = any_nan ? NAN : r_mean(v, n_rows, 0, n1) - r_mean(v, n_rows, n1, n2);
		if (nx == 0 || ny == 0) { p_out[r] = NAN; continue; }
		// 2W = sum over pairs (x_i > y_j: 2, x_i == y_j: 1); ties = sum over tie groups of t^3 - t = sum over values of c^2 - 1
		long long w2 = 0, ties = 0;
		for (int i = 0; i < n; ++i) {
			const double a = v[(unsigned long long)i * n_rows];
			if (!isfinite(a)) continue;
			long long same = 0;
			for (int j = 0; j < n; ++j) {
				const double bj = v[(unsigned long long)j * n_rows];
				if (!isfinite(bj)) continue;
				same += bj == a;
				if (i < n1 && j >= n1) w2 += a > bj ? 2 : (a == bj ? 1 : 0);
			}
			ties += same * same - 1;
		}
		const long long mn = (long long)nx * ny;
		double p;
		if (nx < WILCOX_EXACT_MAX && ny < WILCOX_EXACT_MAX && ties == 0) {
			const long long off = exact_off[nx * WILCOX_EXACT_MAX + ny], w = w2 / 2;
			if (off < 0) { p = NAN; }
			else {
				const double P = 2 * w > mn ? exact_cdf[off + (mn - w)] : exact_cdf[off + w];
				p = fmin(1.0, 2.0 * P);
			}
		} else {
			const double N = (double)(nx + ny);
			double z = 0.5 * (double)w2 - (double)mn / 2.0;
			const double sigma = sqrt(((double)mn / 12.0) * ((N + 1.0) - (double)ties / (N * (N - 1.0))));
			if (!(sigma > 0.0)) { p = NAN; }
			else {
				const double corr = z > 0.0 ? 0.5 : (z < 0.0 ? -0.5 : 0.0);
				z = (z - corr) / sigma;
				p = fmin(erfc(-z / M_SQRT2), erfc(z / M_SQRT2));   // 2 min(pnorm(z), pnorm(z, lower.tail = FALSE))
			}
		}
		p_out[r] = p;
	}
}

// ---- correction -----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) lsq_as_flag_kernel(const double *p, unsigned long long n, unsigned *flag, double *bon, double *bh) {
	for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
		const double v = p[i];
		flag[i] = isnan(v) ? 0u : 1u;
		if (isnan(v)) { bon[i] = v; bh[i] = v; }
	}
}

// the sort's records (lsq_sort.hpp): w0 = the p-value's bits (non-negative doubles sort as their bit patterns), w1 = its index
__global__ void __launch_bounds__(256) lsq_as_compact_kernel(const double *p, unsigned long long n, const unsigned *flag, const unsigned long long *pos,
                                                              unsigned long long *key, unsigned long long *idx) {
	for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
		if (!flag[i]) continue;
		const double v = p[i];
		key[pos[i]] = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);     // -0 sorts as +0
		idx[pos[i]] = i;
	}
}

constexpr unsigned MIN_BLOCK = 4096;      // values per workgroup of the reverse min-scan: 256 lanes x 16

__device__ inline double bh_value(const unsigned long long *key, unsigned long long k, double nd) {
	return (nd / (double)(k + 1)) * __longlong_as_double((long long)key[k]);     // p.adjust: n/i * p[o]
}

__global__ void __launch_bounds__(256) lsq_as_minblock_kernel(const unsigned long long *key, unsigned long long n, double *bmin) {
	__shared__ double lds[4];
	const unsigned long long b0 = (unsigned long long)blockIdx.x * MIN_BLOCK;
	const double nd = (double)n;
	double m = INFINITY;
	for (unsigned q = 0; q < MIN_BLOCK / 256; ++q) {
		const unsigned long long k = b0 + q * 256u + threadIdx.x;
		if (k < n) m = fmin(m, bh_value(key, k, nd));
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) m = fmin(m, __shfl_xor(m, d));
	if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = m;
	__syncthreads();
	if (threadIdx.x == 0) bmin[blockIdx.x] = fmin(fmin(lds[0], lds[1]), fmin(lds[2], lds[3]));
}

// one lane: bmin[b] <- the minimum over the blocks after b (exclusive suffix minimum; a few hundred blocks per million values)
__global__ void lsq_as_minspine_kernel(double *bmin, unsigned long long n_blocks) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	double run = INFINITY;
	for (unsigned long long b = n_blocks; b-- > 0;) { const double v = bmin[b]; bmin[b] = run; run = fmin(run, v); }
}

// the sorted values again: BH = min(1, running minimum from the largest down), Bonferroni = min(1, n p), scattered back
__global__ void __launch_bounds__(256) lsq_as_minapply_kernel(const unsigned long long *key, const unsigned long long *idx, unsigned long long n,
                                                               const double *bcarry, double *bon, double *bh) {
	__shared__ double lds[4];
	const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const unsigned long long k0 = (unsigned long long)blockIdx.x * MIN_BLOCK + threadIdx.x * 16ull;
	const double nd = (double)n;
	double m = INFINITY;
	for (unsigned q = 0; q < 16; ++q) if (k0 + q < n) m = fmin(m, bh_value(key, k0 + q, nd));
	// inclusive suffix minimum over the lanes of the wave, then over the waves after this one
	double suf = m;
#pragma unroll
	for (unsigned d = 1; d < 64; d <<= 1) {
		const double o = __shfl_down(suf, d);
		if (lane + d < 64) suf = fmin(suf, o);
	}
	if (lane == 0) lds[w] = suf;
	__syncthreads();
	double run = bcarry[blockIdx.x];
	for (unsigned q = w + 1; q < 4; ++q) run = fmin(run, lds[q]);
	const double after = __shfl_down(suf, 1);
	if (lane < 63) run = fmin(run, after);
	for (int q = 15; q >= 0; --q) {
		const unsigned long long k = k0 + (unsigned)q;
		if (k >= n) continue;
		const double pv = __longlong_as_double((long long)key[k]);
		run = fmin(run, bh_value(key, k, nd));
		const unsigned i = (unsigned)idx[k];
		bh[i] = fmin(1.0, run);
		bon[i] = fmin(1.0, nd * pv);
	}
}

// [n][cols] row-major (the ABI's layout) -> [cols][n] sample-major, so that lane r reading sample j is a coalesced load
std::vector<double> sample_major(const double *a, unsigned long long n, int cols) {
	std::vector<double> t((size_t)n * (size_t)cols);
	for (unsigned long long r = 0; r < n; ++r)
		for (int j = 0; j < cols; ++j) t[(size_t)j * n + r] = a[(size_t)r * cols + j];
	return t;
}

int finish(lsq_ctx *c) {
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(c->stream));
	return LSQ_OK;
}

// Lower CDF of the Wilcoxon statistic W for (nx, ny): cwilcox's counts built by f(w; a, b) = f(w - b; a - 1, b) + f(w; a, b - 1)
// in doubles, then summed over choose(nx + ny, nx) in order, as pwilcox sums them.
std::vector<double> wilcox_cdf(int nx, int ny) {
	const size_t W = (size_t)nx * ny + 1;
	// F[a][w] over b = 0 .. ny (in place: F[a] holds b - 1's counts until a's turn)
	std::vector<std::vector<double>> F((size_t)nx + 1, std::vector<double>(W, 0.0));
	for (int a = 0; a <= nx; ++a) F[(size_t)a][0] = 1.0;         // b = 0: only W = 0
	for (int b = 1; b <= ny; ++b)
		for (int a = 1; a <= nx; ++a)
			for (size_t w = W; w-- > (size_t)b;) F[(size_t)a][w] += F[(size_t)a - 1][w - (size_t)b];
	double c = 1.0;          // choose(nx + ny, nx)
	for (int q = 1; q <= nx; ++q) c = c * (double)(ny + q) / (double)q;
	c = std::round(c);
	std::vector<double> cdf(W);
	double s = 0.0;
	for (size_t w = 0; w < W; ++w) { s += F[(size_t)nx][w] / c; cdf[w] = s; }
	return cdf;
}

} // namespace

extern "C" {

// Test_AS.r:34-47 (fisher.test per pair of rows)
int lsq_as_fisher(lsq_ctx *c, uint64_t n_tables, const double *cells, double *p) LSQ_API_TRY {
	if (!c || (n_tables && (!cells || !p))) return fail(LSQ_E_ARG, "null argument");
	if (n_tables == 0) return LSQ_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf<double> d_cells, d_p;
	int rc;
	if ((rc = d_cells.upload(cells, (size_t)n_tables * 4, c->stream)) || (rc = d_p.alloc((size_t)n_tables))) return rc;
	hipLaunchKernelGGL(lsq_as_fisher_kernel, dim3(grid_for(c->n_cu, n_tables, 4, 32)), dim3(256), 0, c->stream, d_cells.p, (unsigned long long)n_tables, d_p.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(p, d_p.p, (size_t)n_tables * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	return finish(c);
} LSQ_API_CATCH

// Test_AS.r:89-131 (glm + lrtest per row)
int lsq_as_lrt(lsq_ctx *c, uint64_t n_rows, int n1, int n2, const double *count, const double *total, double *stat, double *p) LSQ_API_TRY {
	if (!c || (n_rows && (!count || !total || !stat || !p))) return fail(LSQ_E_ARG, "null argument");
	if (n1 < 1 || n2 < 1 || n1 > 4096 || n2 > 4096) return fail(LSQ_E_ARG, "replicates per condition must lie in [1, 4096] (n1 = %d, n2 = %d)", n1, n2);
	if (n_rows == 0) return LSQ_OK;
	HIP_TRY(hipSetDevice(c->device));
	const int n = n1 + n2;
	DevBuf<double> d_count, d_total, d_stat, d_p;
	int rc;
	const std::vector<double> hc = sample_major(count, n_rows, n), ht = sample_major(total, n_rows, n);
	if ((rc = d_count.upload(hc.data(), hc.size(), c->stream)) || (rc = d_total.upload(ht.data(), ht.size(), c->stream)) ||
	    (rc = d_stat.alloc((size_t)n_rows)) || (rc = d_p.alloc((size_t)n_rows))) return rc;
	hipLaunchKernelGGL(lsq_as_lrt_kernel, dim3(grid_for(c->n_cu, n_rows, 256, 8)), dim3(256), 0, c->stream, d_count.p, d_total.p, (unsigned long long)n_rows, n1, n2, d_stat.p, d_p.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(stat, d_stat.p, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(p, d_p.p, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	return finish(c);
} LSQ_API_CATCH

// No counterpart in Test_AS.r: the replicate-aware test (beta-binomial model + LRT per row)
int lsq_as_betabin(lsq_ctx *c, uint64_t n_rows, int n1, int n2, const double *count, const double *total,
                   double *mu1, double *mu2, double *rho, double *stat, double *p) LSQ_API_TRY {
	if (!c || (n_rows && (!count || !total || !mu1 || !mu2 || !rho || !stat || !p))) return fail(LSQ_E_ARG, "null argument");
	if (n1 < 1 || n2 < 1 || n1 > 4096 || n2 > 4096) return fail(LSQ_E_ARG, "replicates per condition must lie in [1, 4096] (n1 = %d, n2 = %d)", n1, n2);
	if (n1 + n2 < 3) return fail(LSQ_E_ARG, "the beta-binomial test needs at least 3 samples (n1 + n2 = %d): one shared dispersion and a mean per condition", n1 + n2);
	if (n_rows == 0) return LSQ_OK;
	HIP_TRY(hipSetDevice(c->device));
	const int n = n1 + n2;
	DevBuf<double> d_count, d_total, d_out;
	int rc;
	const std::vector<double> hc = sample_major(count, n_rows, n), ht = sample_major(total, n_rows, n);
	if ((rc = d_count.upload(hc.data(), hc.size(), c->stream)) || (rc = d_total.upload(ht.data(), ht.size(), c->stream)) ||
	    (rc = d_out.alloc((size_t)n_rows * 5))) return rc;
	double *o = d_out.p;
	// the fit's iteration counts differ from row to row: blocks of one wave, so that a long row holds up 63 others and no more
	hipLaunchKernelGGL(lsq_as_betabin_kernel, dim3(grid_for(c->n_cu, n_rows, 64, 32)), dim3(64), 0, c->stream, d_count.p, d_total.p, (unsigned long long)n_rows, n1, n2,
	                   o, o + n_rows, o + 2 * n_rows, o + 3 * n_rows, o + 4 * n_rows);
	HIP_TRY(hipGetLastError());
	double *const host[5] = {mu1, mu2, rho, stat, p};
	for (int q = 0; q < 5; ++q) HIP_TRY(hipMemcpyAsync(host[q], o + (size_t)q * n_rows, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	return finish(c);
} LSQ_API_CATCH

// developer entry (lesseq_hip_dev.h): sum_j l_j(mu_r, rho_r) per row through the fit's own device function
int lsq_debug_as_bb_loglik(lsq_ctx *c, uint64_t n_rows, int n_samples, const double *y, const double *n, const double *mu, const double *rho, double *out) LSQ_API_TRY {
	if (!c || (n_rows && (!y || !n || !mu || !rho || !out))) return fail(LSQ_E_ARG, "null argument");
	if (n_samples < 1 || n_samples > 8192) return fail(LSQ_E_ARG, "samples per row must lie in [1, 8192] (%d)", n_samples);
	if (n_rows == 0) return LSQ_OK;
	HIP_TRY(hipSetDevice(c->device));
	DevBuf<double> d_y, d_n, d_mu, d_rho, d_out;
	int rc;
	const std::vector<double> hy = sample_major(y, n_rows, n_samples), hn = sample_major(n, n_rows, n_samples);
	if ((rc = d_y.upload(hy.data(), hy.size(), c->stream)) || (rc = d_n.upload(hn.data(), hn.size(), c->stream)) ||
	    (rc = d_mu.upload(mu, (size_t)n_rows, c->stream)) || (rc = d_rho.upload(rho, (size_t)n_rows, c->stream)) || (rc = d_out.alloc((size_t)n_rows))) return rc;
	hipLaunchKernelGGL(lsq_as_bb_loglik_kernel, dim3(grid_for(c->n_cu, n_rows, 256, 8)), dim3(256), 0, c->stream, (const double *)d_y.p, (const double *)d_n.p,
	                   (unsigned long long)n_rows, n_samples, (const double *)d_mu.p, (const double *)d_rho.p, d_out.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	return finish(c);
} LSQ_API_CATCH

// Test_AS.r:162-175 (mean difference + wilcox.test per row)
int lsq_as_wilcox(lsq_ctx *c, uint64_t n_rows, int n1, int n2, const double *value, double *diff, double *p) LSQ_API_TRY {
	if (!c || (n_rows && (!value || !diff || !p))) return fail(LSQ_E_ARG, "null argument");
	if (n1 < 1 || n2 < 1 || n1 > 4096 || n2 > 4096) return fail(LSQ_E_ARG, "replicates per condition must lie in [1, 4096] (n1 = %d, n2 = %d)", n1, n2);
	if (n_rows == 0) return LSQ_OK;
	HIP_TRY(hipSetDevice(c->device));
	const int n = n1 + n2;
	// exact tables for every (nx, ny) that a row can have after its non-finite values are dropped
	std::vector<long long> off((size_t)WILCOX_EXACT_MAX * WILCOX_EXACT_MAX, -1);
	std::vector<double> cdf;
	for (uint64_t r = 0; r < n_rows; ++r) {
		int nx = 0, ny = 0;
		for (int j = 0; j < n; ++j) if (std::isfinite(value[(size_t)r * n + j])) { if (j < n1) ++nx; else ++ny; }
		if (nx == 0 || ny == 0 || nx >= WILCOX_EXACT_MAX || ny >= WILCOX_EXACT_MAX) continue;
		long long &o = off[(size_t)nx * WILCOX_EXACT_MAX + ny];
		if (o >= 0) continue;
		o = (long long)cdf.size();
		const std::vector<double> t = wilcox_cdf(nx, ny);
		cdf.insert(cdf.end(), t.begin(), t.end());
	}
	DevBuf<double> d_value, d_cdf, d_diff, d_p;
	DevBuf<long long> d_off;
	int rc;
	const std::vector<double> hv = sample_major(value, n_rows, n);
	if ((rc = d_value.upload(hv.data(), hv.size(), c->stream)) || (rc = d_off.upload(off.data(), off.size(), c->stream)) ||
	    (rc = d_cdf.upload(cdf.data(), cdf.size(), c->stream)) || (rc = d_diff.alloc((size_t)n_rows)) || (rc = d_p.alloc((size_t)n_rows))) return rc;
	hipLaunchKernelGGL(lsq_as_wilcox_kernel, dim3(grid_for(c->n_cu, n_rows, 256, 8)), dim3(256), 0, c->stream, d_value.p, (unsigned long long)n_rows, n1, n2,
	                   (const long long *)d_off.p, (const double *)d_cdf.p, d_diff.p, d_p.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(diff, d_diff.p, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(p, d_p.p, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	return finish(c);
} LSQ_API_CATCH

// Test_AS.r:45,129,173 (p.adjust, "bonferroni" and "BH")
int lsq_as_adjust(lsq_ctx *c, uint64_t n, const double *p, double *p_bonferroni, double *p_bh) LSQ_API_TRY {
	if (!c || (n && (!p || !p_bonferroni || !p_bh))) return fail(LSQ_E_ARG, "null argument");
	if (n >= 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32 - 2 p-values");
	uint64_t n_valid = 0;
	for (uint64_t i = 0; i < n; ++i) {
		if (std::isnan(p[i])) continue;
		if (p[i] < 0.0) return fail(LSQ_E_ARG, "p-value %llu is negative (%g)", (unsigned long long)i, p[i]);
		++n_valid;
	}
	if (n_valid <= 1) {          // p.adjust returns p unchanged
		if (n) { memmove(p_bonferroni, p, (size_t)n * sizeof(double)); memmove(p_bh, p, (size_t)n * sizeof(double)); }
		return LSQ_OK;
	}
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	const unsigned nb = grid_for(n_valid, MIN_BLOCK);
	DevBuf<double> d_p, d_bon, d_bh, d_bmin;
	DevBuf<unsigned> d_flag;
	DevBuf<unsigned long long> d_pos;
	ScanScratch S;            // of the flag scan over all n values; the sort's scans (over its digit table) have B's own
	SortBuf B;
	int rc;
	if ((rc = d_p.upload(p, (size_t)n, st)) || (rc = d_bon.alloc((size_t)n)) || (rc = d_bh.alloc((size_t)n)) || (rc = d_flag.alloc((size_t)n)) ||
	    (rc = d_pos.alloc((size_t)n + 1)) || (rc = B.reserve(n_valid)) || (rc = d_bmin.alloc(nb)) || (rc = S.reserve(n))) return rc;
	const unsigned g = grid_for(c->n_cu, n, 256, 16);
	hipLaunchKernelGGL(lsq_as_flag_kernel, dim3(g), dim3(256), 0, st, (const double *)d_p.p, (unsigned long long)n, d_flag.p, d_bon.p, d_bh.p);
	if ((rc = device_scan<1, true>(S, d_flag.p, n, d_pos.p, st))) return rc;
	hipLaunchKernelGGL(lsq_as_compact_kernel, dim3(g), dim3(256), 0, st, (const double *)d_p.p, (unsigned long long)n, (const unsigned *)d_flag.p,
	                   (const unsigned long long *)d_pos.p, B.w0[B.cur].p, B.w1[B.cur].p);
	static const unsigned KEY_DIGITS[8] = {0, 8, 16, 24, 32, 40, 48, 56};      // all of w0; the index in w1 rides along
	if ((rc = device_radix_sort(B, KEY_DIGITS, 8, st))) return rc;
	const unsigned long long *key = B.w0[B.cur].p, *idx = B.w1[B.cur].p;
	hipLaunchKernelGGL(lsq_as_minblock_kernel, dim3(nb), dim3(256), 0, st, key, (unsigned long long)n_valid, d_bmin.p);
	hipLaunchKernelGGL(lsq_as_minspine_kernel, dim3(1), dim3(64), 0, st, d_bmin.p, (unsigned long long)nb);
	hipLaunchKernelGGL(lsq_as_minapply_kernel, dim3(nb), dim3(256), 0, st, key, idx, (unsigned long long)n_valid, (const double *)d_bmin.p, d_bon.p, d_bh.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(p_bonferroni, d_bon.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(p_bh, d_bh.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
	return finish(c);
} LSQ_API_CATCH

} // extern "C"
