// posterior_dev.hpp - products of the per-row posteriors of the last save_gamma E-step, computed where the rows lie (DESIGN.md,
// "Posterior products on the device").  Included from engine.hip; the host side is in engine_products.hpp (smcpp_posterior_*).
//
// Source of every kernel: `rows` [L + 1][Mp] fp64, one row per caller's row (d_gamma_rows of the contig, or merged_gamma(c) where long
// rows were cut), states contiguous; row 0 of that block is unset: column 0 is `g0` [Mp] (gamma0 of the contig).  The padding states
// M .. Mp - 1 are never read.  A column selection is (start, step, ncols): column j of a product is row start + j * step.
//
//   k_post_columns   [M x ncols] fp64 or fp32, gamma or gamma / column sum, a tiled transpose through LDS; the column sums
//   k_post_summary   per column: sum, first argmax, sum_m w_m p_m, up to 8 quantile states - O(ncols) output
//   k_post_windows   [M x n_windows]: the average of p over windows of W base pairs, one wavefront per window, no atomics
//
// Every sum over the states of a column and every sum over the rows of a window is a chain of plain additions in ascending order
// carried by ONE thread, so no result depends on the launch shape.  All three are bound by HBM bandwidth.
#pragma once

namespace smcpp_dev {

struct PostSel { long long start, step, ncols; };
struct PostLevels { int nq; double q[8]; };

__device__ __forceinline__ const double *post_row(const double *__restrict__ rows, const double *__restrict__ g0, int Mp, long long r) {
    return r == 0 ? g0 : rows + (size_t)r * Mp;
}

// ---- columns ----------------------------------------------------------------------------------------------------------------
// A workgroup owns PC_TL columns and walks the states in tiles of PC_TM.  A tile is read with the states along the lanes (256 B per
// row, two rows per wavefront) and written out with the columns along the lanes (512 B per state).  LDS rows are padded to an odd
// number of doubles: an fp64 element covers two banks, so the 32 lanes of a half wavefront that read one state of 32 columns hit
// 2 * 33 * l mod 64 - 32 distinct even banks and their odd neighbours; the row-wise stores are consecutive.
// When the sums are needed (normalisation or the colsum output) a first walk over the tiles adds each column up - thread l owns column
// l, states ascending - and the second walk re-reads the tiles (64 x Mp doubles: they are still in L2).
constexpr int PC_TL = 64, PC_TM = 32, PC_LD = PC_TM + 1;

template <typename OutT>
__global__ __launch_bounds__(256) void k_post_columns(int M, int Mp, PostSel sel, const double *__restrict__ rows, const double *__restrict__ g0,
                                                      int need_sum, int normalize, OutT *__restrict__ out, double *__restrict__ colsum) {
    __shared__ double tile[PC_TL * PC_LD];
    __shared__ double ssum[PC_TL];
    const int t = threadIdx.x;
    const long long j0 = (long long)blockIdx.x * PC_TL;
    const int lm = t % PC_TM, ll = t / PC_TM;          // load: 32 states x 8 columns per step
    const int sl = t % PC_TL, sm = t / PC_TL;          // store: 64 columns x 4 states per step
    auto load = [&](int m0) {
        const int m = m0 + lm;
        for (int l = ll; l < PC_TL; l += 256 / PC_TM) {
            const long long j = j0 + l;
            if (j < sel.ncols && m < M) tile[l * PC_LD + lm] = post_row(rows, g0, Mp, sel.start + j * sel.step)[m];
        }
    };
    if (need_sum) {
        double s = 0.0;
        for (int m0 = 0; m0 < M; m0 += PC_TM) {
            load(m0);
            __syncthreads();
            if (t < PC_TL && j0 + t < sel.ncols) {
                const int mt = min(PC_TM, M - m0);
                for (int i = 0; i < mt; ++i) s += tile[t * PC_LD + i];
            }
            __syncthreads();
        }
        if (t < PC_TL) {
            ssum[t] = s;
            if (colsum && j0 + t < sel.ncols) colsum[j0 + t] = s;
        }
        __syncthreads();
    }
    if (!out) return;
    const double div = normalize ? ssum[sl] : 1.0;
    for (int m0 = 0; m0 < M; m0 += PC_TM) {
        load(m0);
        __syncthreads();
        if (j0 + sl < sel.ncols)
            for (int m = sm; m < PC_TM && m0 + m < M; m += 256 / PC_TL) {
                double v = tile[sl * PC_LD + m];
                if (normalize) v = v / div;
                out[(size_t)(m0 + m) * sel.ncols + j0 + sl] = (OutT)v;
            }
        __syncthreads();
    }
}

// ---- summary ----------------------------------------------------------------------------------------------------------------
// A workgroup owns 256 columns, one per thread, and walks the states in tiles of 16 staged through LDS (read with the states along the
// lanes, 128 B per row; consumed with the columns along the lanes, row stride 17 doubles: odd, as above).  First walk: the sum and the
// first maximum (the rule of k_gamma_argmax).  Second walk, only when weights or levels are given: p_m = g_m / sum, the running sum of
// p (what np.cumsum does), sum_m w_m p_m, and per level the first state whose running sum reaches it (the last state if rounding
// keeps the total below the level).
constexpr int PS_TL = 256, PS_TM = 16, PS_LD = PS_TM + 1;

__global__ __launch_bounds__(256) void k_post_summary(int M, int Mp, PostSel sel, const double *__restrict__ rows, const double *__restrict__ g0,
                                                      const double *__restrict__ w, PostLevels lv, double *__restrict__ colsum,
                                                      int *__restrict__ argmax, double *__restrict__ mean, int *__restrict__ qstate) {
    __shared__ double tile[PS_TL * PS_LD];
    const int t = threadIdx.x;
    const long long j0 = (long long)blockIdx.x * PS_TL, j = j0 + t;
    const bool live = j < sel.ncols;
    const int lm = t % PS_TM, ll = t / PS_TM;          // load: 16 states x 16 columns per step
    auto load = [&](int m0) {
        const int m = m0 + lm;
        for (int l = ll; l < PS_TL; l += 256 / PS_TM) {
            const long long jj = j0 + l;
            if (jj < sel.ncols && m < M) tile[l * PS_LD + lm] = post_row(rows, g0, Mp, sel.start + jj * sel.step)[m];
        }
    };
    double s = 0.0, bv = 0.0;
    int best = 0;
    for (int m0 = 0; m0 < M; m0 += PS_TM) {
        load(m0);
        __syncthreads();
        if (live) {
            const int mt = min(PS_TM, M - m0);
            for (int i = 0; i < mt; ++i) {
                const double v = tile[t * PS_LD + i];
                s += v;
                if (m0 + i == 0) bv = v;
                else if (v > bv) { bv = v; best = m0 + i; }
            }
        }
        __syncthreads();
    }
    if (live) {
        if (colsum) colsum[j] = s;
        if (argmax) argmax[j] = best;
    }
    if (!w && lv.nq == 0) return;
    double cum = 0.0, mu = 0.0;
    int qs[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) qs[k] = -1;
    for (int m0 = 0; m0 < M; m0 += PS_TM) {
        load(m0);
        __syncthreads();
        if (live) {
            const int mt = min(PS_TM, M - m0);
            for (int i = 0; i < mt; ++i) {
                const double p = tile[t * PS_LD + i] / s;
                cum += p;
                if (w) mu += w[m0 + i] * p;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < lv.nq && qs[k] < 0 && cum >= lv.q[k]) qs[k] = m0 + i;
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (w && mean) mean[j] = mu;
    if (qstate) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < lv.nq) qstate[(size_t)k * sel.ncols + j] = qs[k] < 0 ? M - 1 : qs[k];
    }
}

// ---- windows ----------------------------------------------------------------------------------------------------------------
// P [L + 1] are the prefix positions of the caller's rows (P[0] = 0, P[l] = s_1 + .. + s_l): row l >= 1 covers base pairs
// [P[l-1], P[l]).  Window w covers [w W, min((w + 1) W, P[L])).  One wavefront per (window, group of 64 states): lane = state; it
// finds the first row that reaches into the window by bisection in P and adds overlap * gamma[l] / colsum[l] over its rows in ascending
// order, then divides by the covered base pairs.  `colsum` [L + 1] comes from k_post_summary over all rows, so p is the same number
// the other products use.  A workgroup of four wavefronts takes PW_WPB consecutive windows and hands the results over through LDS,
// so that the stores run along the window axis (128 B per state) instead of one double per state.
constexpr int PW_WPB = 16, PW_LD = PW_WPB + 1;

__global__ __launch_bounds__(256) void k_post_windows(int M, int Mp, long long L, long long W, long long nwin, const long long *__restrict__ P,
                                                      const double *__restrict__ rows, const double *__restrict__ colsum,
                                                      double *__restrict__ out) {
    __shared__ double res[64 * PW_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long w0 = (long long)blockIdx.x * PW_WPB;
    const int m0 = blockIdx.y * 64, m = m0 + lane;
    const long long total = P[L];
    for (int k = 0; k < PW_WPB / 4; ++k) {
        const int wi = wave * (PW_WPB / 4) + k;
        const long long w = w0 + wi;
        if (w >= nwin) break;                                   // (the same for every lane of the wavefront)
        const long long lo = w * W, hi = min(lo + W, total);
        long long a = 1, b = L;                                 // first row l >= 1 with P[l] > lo (it exists: lo < P[L])
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if (P[mid] > lo) b = mid; else a = mid + 1;
        }
        double acc = 0.0;
        long long p0 = P[a - 1];
        for (long long l = a; l <= L && p0 < hi; ++l) {
            const long long p1 = P[l];
            const long long ov = min(p1, hi) - max(p0, lo);
            if (m < M) acc += (double)ov * (rows[(size_t)l * Mp + m] / colsum[l]);
            p0 = p1;
        }
        res[lane * PW_LD + wi] = acc / (double)(hi - lo);
    }
    __syncthreads();
    const int wi = t % PW_WPB;
    if (w0 + wi < nwin)
        for (int mm = t / PW_WPB; mm < 64 && m0 + mm < M; mm += 256 / PW_WPB)
            out[(size_t)(m0 + mm) * nwin + w0 + wi] = res[mm * PW_LD + wi];
}

}  // namespace smcpp_dev
