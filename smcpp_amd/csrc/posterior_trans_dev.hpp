// posterior_trans_dev.hpp - posterior TRANSITION products of the last save_gamma E-step: per row and per window the expected number of
// positions at which the hidden state stays, moves up (to a higher index = older state) or moves down ("Posterior
// transition products").  Included from engine.hip behind chains_ss.hpp (the scan steps), walk_dev.hpp (the leaves of a row walk)
// and posterior_dev.hpp (PostSel); the host side is in engine_products.hpp (smcpp_posterior_transitions / _transition_windows).
//
// For a position p of a row with emission vector e, forward vector x_{p-1} before it and backward vector y_p after it,
//     xi_p(i, j) = x_{p-1}(i) T(i, j) e(j) y_p(j) / Z_p,     stay = sum_i xi(i, i),  up = sum_{i<j} xi(i, j),  down = sum_{i>j} xi(i, j).
// The forward scan step is written in three addends,
//     (T^T u)_j = d_j u_j  +  g_j sum_{i>j} u_i  +  (c0 sum_{i<j} u_i + Z_j),
// which are the mass that reaches state j from j itself, from above and from below: with w = e o y_p the three products are the dot
// products of w with the addends of u = x_{p-1}, and Z_p is their sum.  No M x M object is formed: O(M) per position.
//
//   k_post_transitions          one wavefront per ENGINE row (a caller's row, or a piece of one where long rows were cut): [3][L + 1]
//   k_post_transitions_select   the pieces of a caller's row added up, a column selection taken: [3][ncols]
//   k_post_transition_windows   [3][n_windows]: expected counts per window of W base pairs, one wavefront per window
//
// x and y start from what the E-step stored - the float alpha at the row's start, beta at its end - and are advanced through the
// row by ss_fwd_step's arithmetic / ss_bwd_step, rescaled at every step (every position is normalised by its own Z_p, so the scales
// cancel).  A row is walked in BLOCKS of at most 64 positions: the forward walk of a block parks the three addends of every position
// as floats in the wavefront's own scratch, the backward walk multiplies them in.  A row of more than one block first runs forward
// once and keeps x at every block start (fp64 checkpoints in the wavefront's scratch), then takes its blocks from the last to the
// first: 3 s - 1 steps for s positions, and the scratch is 64 positions + s / 64 vectors however long the row is.
// Every sum runs in a fixed order - the positions of a row descending in ONE wavefront, the pieces of a row and the rows of a
// window ascending in one thread -, with a compensated accumulator where thousands of terms meet, so no result depends on the
// launch shape or on what ran before.  No atomics.
#pragma once

namespace smcpp_dev {

struct PtArgs {
    WalkRows w;
    int L;                      // ENGINE rows of the contig (rows 1 .. L; row 0 is column 0)
    int nck;                    // checkpoint vectors per wavefront (blocks of the longest row - 1)
    float *park;                // [wavefronts][64][3][MS]
    double *ckpt;               // [wavefronts][nck][MS]
    double *out;                // [3][L + 1]
};

constexpr int PT_BLK = 64;

// The addends of T^T x, state by state (ss_fwd_step's scans, chains_ss.hpp), handed to `sink(k, stay, down, low, Z)`; S = sum x.  The
// addend from below is c0 low + Z: low = sum_{i<j} x_i meets the uniform mix, Z the Phi' part of the upper triangle.
template <int NPL, typename Sink>
__device__ __forceinline__ void pt_fwd_parts(const SsFwdC<NPL> &c, const double (&x)[NPL], double &S, Sink sink) {
    double lp[NPL], w[NPL];
    lp[0] = x[0];
    w[0] = c.b[0] * x[0];
#pragma unroll
    for (int k = 1; k < NPL; ++k) {
        lp[k] = lp[k - 1] + x[k];
        w[k] = __builtin_fma(c.a[k], w[k - 1], c.b[k] * x[k]);
    }
    double p_ = lp[NPL - 1], z_ = w[NPL - 1];
    {
        double tp, tz;
        tp = dpp0<DPP_SHR1>(p_); tz = dpp0<DPP_SHR1>(z_); p_ += tp; z_ = __builtin_fma(c.lv[0], tz, z_);
        tp = dpp0<DPP_SHR2>(p_); tz = dpp0<DPP_SHR2>(z_); p_ += tp; z_ = __builtin_fma(c.lv[1], tz, z_);
        tp = dpp0<DPP_SHR4>(p_); tz = dpp0<DPP_SHR4>(z_); p_ += tp; z_ = __builtin_fma(c.lv[2], tz, z_);
        tp = dpp0<DPP_SHR8>(p_); tz = dpp0<DPP_SHR8>(z_); p_ += tp; z_ = __builtin_fma(c.lv[3], tz, z_);
        tp = dpp0<DPP_BC15>(p_); tz = dpp0<DPP_BC15>(z_); p_ = __builtin_fma(c.c15, tp, p_); z_ = __builtin_fma(c.lv[4], tz, z_);
        tp = dpp0<DPP_BC31>(p_); tz = dpp0<DPP_BC31>(z_); p_ = __builtin_fma(c.c31, tp, p_); z_ = __builtin_fma(c.lv[5], tz, z_);
    }
    const double li = p_;
    S = lane_get(li, 63);
    const double LIp = dpp0<DPP_WSHR1>(z_);
    const double lex = li - lp[NPL - 1];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const double incl = lex + lp[k];                                   // sum_{i <= j} x_i
        const double Z = (k == 0) ? LIp : __builtin_fma(c.cumA[k - 1 < 0 ? 0 : k - 1], LIp, w[k - 1 < 0 ? 0 : k - 1]);
        sink(k, c.d[k] * x[k], c.g[k] * (S - incl), incl - x[k], Z);
    }
}
// The three addends of T^T x - stay, from above, from below - handed to `sink(k, stay, down, up)`.
template <int NPL, typename Sink>
__device__ __forceinline__ void pt_fwd_addends(const SsFwdC<NPL> &c, double c0, const double (&x)[NPL], double &S, Sink sink) {
    pt_fwd_parts<NPL>(c, x, S, [&](int k, double s0, double s1, double low, double Z) { sink(k, s0, s1, __builtin_fma(c0, low, Z)); });
}

template <int NPL>
__global__ __launch_bounds__(256) void k_post_transitions(SsArgs sa, PtArgs a, int nwaves) {
    constexpr int MS = 64 * NPL;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const int M = a.w.M;
    const size_t LD = (size_t)a.L + 1;
    float *park = a.park + (size_t)gw * PT_BLK * 3 * MS;
    double *ckpt = a.ckpt + (size_t)gw * a.nck * MS;
    if (gw == 0 && lane < 3) a.out[lane * LD] = 0.0;                       // column 0: no transition enters it
    for (int r = 1 + gw; r <= a.L; r += nwaves) {
        const WalkRow wr = walk_row(a.w, r);
        const int span = wr.span;
        const int nblk = (span + PT_BLK - 1) / PT_BLK;
        // ---- rows of more than one block: x at the start of blocks 1 .. nblk - 1 ----
        if (nblk > 1) {
            SsFwdC<NPL> c;
            ss_load_fwd<NPL>(sa, lane, c);
            // (x and e in ONE hand-written loop, and the backward walk's e with its state table below: with the leaves of walk_dev.hpp
            // in these two places the kernel passes 168 registers at four states per lane, and a third wavefront per SIMD is lost)
            double x[NPL], ev[NPL], part = 0.0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const int st = lane * NPL + k;
                const bool live = st < M;
                x[k] = live ? (double)wr.ap[live ? st : 0] : 0.0;
                ev[k] = live ? wr.ek[live ? st : 0] : 0.0;
                part += x[k];
            }
            const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
            for (int k = 0; k < NPL; ++k) x[k] *= i0;
            walk_checkpoints<NPL, PT_BLK>(x, ckpt, nblk, lane, [&](const double (&u)[NPL], double (&out)[NPL], double &S) {
                pt_fwd_addends<NPL>(c, sa.c0, u, S, [&](int k, double s0, double s1, double s2) { out[k] = ev[k] * (s0 + s1 + s2); });
            });
        }
        // ---- the blocks, last to first: y carried in a running scale across them ----
        double h[NPL];
        walk_load_norm<NPL, true>(a.w.beta + wr.row * a.w.Mp, M, lane, h);
        double acc[3] = {0.0, 0.0, 0.0}, cmp[3] = {0.0, 0.0, 0.0};
        for (int b = nblk - 1; b >= 0; --b) {
            const int len = min(PT_BLK, span - b * PT_BLK);
            {
                // forward through the block: the addends of x_{p-1} of every position p of the block
                SsFwdC<NPL> c;
                ss_load_fwd<NPL>(sa, lane, c);
                double x[NPL], ev[NPL];
                walk_block_start<NPL>(wr.ap, ckpt, b, M, lane, x);
                walk_load<NPL>(wr.ek, M, lane, ev);
                for (int t = 0; t < len; ++t) {
                    double out[NPL], S;
                    float *pk = park + (size_t)t * 3 * MS + lane * NPL;
                    pt_fwd_addends<NPL>(c, sa.c0, x, S, [&](int k, double s0, double s1, double s2) {
                        // (parked as floats, as the forward vectors of k_gamma_rows_scan are; Z_p is formed from the same three
                        // floats, so a position's three shares still add up to one)
                        pk[k] = (float)s0; pk[MS + k] = (float)s1; pk[2 * MS + k] = (float)s2;
                        out[k] = ev[k] * (s0 + s1 + s2);
                    });
                    walk_rescale<NPL>(x, out, (float)S);
                }
            }
            // the parked addends are read back by OTHER lanes of this wavefront (reversed state order): the stores have to be
            // acknowledged first (one CU, one vector L1: a workgroup-scope fence is a wait, no cache maintenance)
            __threadfence_block();
            {
                SsBwdC<NPL> c;
                ss_load_bwd<NPL>(sa, lane, c);
                double ev[NPL];
                int st[NPL];
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    st[k] = MS - 1 - (lane * NPL + k);
                    const bool live = st[k] < M;
                    ev[k] = live ? wr.ek[live ? st[k] : 0] : 0.0;
                }
                for (int t = len - 1; t >= 0; --t) {
                    const float *pk = park + (size_t)t * 3 * MS;
                    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
#pragma unroll
                    for (int k = 0; k < NPL; ++k) {
                        const double w = ev[k] * h[k];
                        p0 = __builtin_fma((double)pk[st[k]], w, p0);
                        p1 = __builtin_fma((double)pk[MS + st[k]], w, p1);
                        p2 = __builtin_fma((double)pk[2 * MS + st[k]], w, p2);
                    }
                    const double d0 = wave_sum_dpp(p0), d1 = wave_sum_dpp(p1), d2 = wave_sum_dpp(p2);
                    const double Z = (d0 + d1) + d2;
                    pt_add(acc[0], cmp[0], d0 / Z);
                    pt_add(acc[1], cmp[1], d2 / Z);                                // up: the addend that comes from below
                    pt_add(acc[2], cmp[2], d1 / Z);                                // down: the addend that comes from above
                    if (t > 0 || b > 0) {
                        double out[NPL];
                        float Sw;
                        ss_bwd_step<NPL>(c, h, ev, out, Sw);
                        walk_rescale<NPL>(h, out, Sw);
                    }
                }
            }
            // (the next block's forward walk overwrites the scratch this block's backward walk has just read: every load above has
            // delivered its value - the sums depend on them - before the wavefront gets there)
        }
        if (lane < 3) a.out[lane * LD + r] = lane == 0 ? acc[0] + cmp[0] : lane == 1 ? acc[1] + cmp[1] : acc[2] + cmp[2];
    }
}

// Column j of the selection = caller's row l = start + j step: the sum of its pieces first[l] .. first[l + 1] - 1 (ascending, one
// thread; first == nullptr: no row was cut, the piece is the row).  eng [3][Le + 1] -> out [3][ncols].
__global__ __launch_bounds__(256) void k_post_transitions_select(PostSel sel, long long Le, const int *__restrict__ first,
                                                                 const double *__restrict__ eng, double *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= sel.ncols) return;
    const long long l = sel.start + j * sel.step;
    const long long p0 = first ? first[l] : l, p1 = first ? first[l + 1] : l + 1;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const double *src = eng + (size_t)x * (Le + 1);
        double s = 0.0, c = 0.0;
        for (long long p = p0; p < p1; ++p) pt_add(s, c, src[p]);
        out[(size_t)x * sel.ncols + j] = s + c;
    }
}

// P [L + 1]: prefix positions of the caller's rows (k_post_windows).  out[x][w] = sum_l overlap(l, w) / s_l * v[x][l]: a row is
// apportioned uniformly over its base pairs.  One wavefront per window: it finds the first row that reaches into the window by
// bisection in P; lanes 0 .. 2 add the rows up in ascending order, one product each.  v [3][L + 1] (all caller's rows).
__global__ __launch_bounds__(256) void k_post_transition_windows(long long L, long long W, long long nwin, const long long *__restrict__ P,
                                                                 const double *__restrict__ v, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nwin) return;
    const long long total = P[L];
    const long long lo = w * W, hi = min(lo + W, total);
    long long a = 1, b = L;                                     // first row l >= 1 with P[l] > lo (it exists: lo < P[L])
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (P[mid] > lo) b = mid; else a = mid + 1;
    }
    if (lane >= 3) return;
    const double *src = v + (size_t)lane * (L + 1);
    double s = 0.0, c = 0.0;
    long long p0 = P[a - 1];
    for (long long l = a; l <= L && p0 < hi; ++l) {
        const long long p1 = P[l];
        const long long ov = min(p1, hi) - max(p0, lo);
        pt_add(s, c, (double)ov * (src[l] / (double)(p1 - p0)));
        p0 = p1;
    }
    out[(size_t)lane * nwin + w] = s + c;
}

}  // namespace smcpp_dev
