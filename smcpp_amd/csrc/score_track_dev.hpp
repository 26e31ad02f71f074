// score_track_dev.hpp - the SCORE track of the last save_gamma E-step: per row and per window the derivative of the log-likelihood
// with respect to every seeded direction of the model ("Score track").  Included from engine.hip behind walk_dev.hpp
// (pt_add, the leaves of the row walk), posterior_trans_dev.hpp (pt_fwd_addends) and posterior_dev.hpp (PostSel); the host side
// is in engine_products.hpp (smcpp_score_rows / _windows).
//
// For a position p of a row with key k, emission vector e = E[k], forward vector x_{p-1} before it and backward vector y_p after it,
//     xi_p(i, j) = x_{p-1}(i) T(i, j) e(j) y_p(j) / Z_p,     gamma_p(j) = sum_i xi_p(i, j),
//     u_p[d] = sum_ij xi_p(i, j) dT_d(i, j) / T(i, j)  +  sum_j gamma_p(j) dE_d[k](j) / E[k](j)        (transition + emission part),
// and position 0 adds sum_m gamma_0(m) dpi_d(m) / pi(m) (initial part).  Unlike stay / up / down this needs the M x M object: with
// w_p = e o y_p the wavefront adds x_{p-1}(i) w_p(j) / Z_p into O(i, j) at every position of the row and contracts ONCE per row,
//     transition[d] = sum_ij O(i, j) dT_d(i, j),      emission[d] = sum_j g(j) G_E,d[k](j),   g = sum_p gamma_p.
// The lane of state j keeps column j of O in 64 fp64 registers, so the kernel exists at one state per lane (M <= 64) only.
//
//   k_score_rows      one wavefront per ENGINE row (a caller's row, or a piece of one where long rows were cut): [3][nder][L + 1]
//   k_score_select    the pieces of a caller's row added up, a column selection taken: [3][nder][ncols] or the total [nder][ncols]
//   k_score_windows   [nder][n_windows]: a row apportioned uniformly over its base pairs, one wavefront per window
//
// The walk is k_post_transitions<1>'s, on the same leaves (walk_dev.hpp): blocks of at most 64 positions, fp64 checkpoints of x
// at the block starts of longer rows,
// forward from the stored float alpha, backward from the stored beta, rescaled at every step (every position is normalised by its
// own Z_p).  The forward walk of a block parks x_{p-1} and T^T x_{p-1} of every position as floats in the wavefront's own 32 KB of
// LDS (four wavefronts of a workgroup: 128 of the 160 KB); the backward walk reads T^T x_{p-1} at its own state (Z_p and gamma_p
// come from the same floats, so a position's gamma sums to one) and x_{p-1} at EVERY state - all lanes read the same address, a
// broadcast without bank conflicts.
// Every sum runs in a fixed order: the positions of a row descending in one wavefront, the states in the wavefront reduction, the
// pieces of a row and the rows of a window ascending in one thread.  The terms of O(i, j) are products of probabilities, none
// negative, so its plain fp64 sum over n positions is off by at most n 2^-53 of its value; g and every sum of SIGNED terms (pieces,
// windows) are compensated (pt_add).  No atomics.
#pragma once

namespace smcpp_dev {

struct ScArgs {
    WalkRows w;
    int L;                      // ENGINE rows of the contig (rows 1 .. L; row 0 is column 0)
    int nck;                    // checkpoint vectors per wavefront (blocks of the longest row - 1)
    int nder;                   // directions
    const double *gamma0;       // [Mp] the contig's column 0 as stored (proportional to gamma_0)
    const double *Gpi;          // [nder][64]      dpi_d / pi, zero beyond M
    const double *dT;           // [nder][64][64]  dT_d(i, j), j fastest, zero beyond M
    const double *GE;           // [K][nder][64]   dE_d[k] / E[k], zero beyond M
    double *ckpt;               // [wavefronts][nck][64]
    double *out;                // [3][nder][L + 1]: initial, emission, transition
};

constexpr int SC_BLK = 64;                                       // positions per block
constexpr int SC_LDS_BYTES = 4 * 2 * SC_BLK * 64 * (int)sizeof(float);   // a workgroup's parked vectors

__global__ __launch_bounds__(256) void k_score_rows(SsArgs sa, ScArgs a, int nwaves) {
    extern __shared__ float sc_lds[];                            // [4 wavefronts][2][SC_BLK][64]: x_{p-1} | T^T x_{p-1}
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;                                    // (no workgroup barrier below: the LDS of a wavefront is its own)
    const int M = a.w.M, nder = a.nder;
    const size_t LD = (size_t)a.L + 1;
    float *px = sc_lds + (size_t)(threadIdx.x >> 6) * 2 * SC_BLK * 64;
    float *ptx = px + SC_BLK * 64;
    double *ckpt = a.ckpt + (size_t)gw * a.nck * 64;
    const int st = 63 - lane;                                    // the backward walk holds the states reversed
    if (gw == 0) {
        // column 0: the initial part alone.  The stored column 0 is the reference's alpha_0 o beta_0 with beta_0 / sum beta_0
        // (hmm.cpp:150): proportional to gamma_0, not normalised - it is normalised here, as every xi_p is by its Z_p
        double g0v[1];
        walk_load<1>(a.gamma0, M, lane, g0v);
        const double g0 = g0v[0] / wave_sum_dpp(g0v[0]);
        for (int d = 0; d < nder; ++d) {
            const double s = wave_sum_dpp(g0 * a.Gpi[(size_t)d * 64 + lane]);
            if (lane < 3) a.out[((size_t)lane * nder + d) * LD] = lane == 0 ? s : 0.0;
        }
    }
    for (int r = 1 + gw; r <= a.L; r += nwaves) {
        const WalkRow wr = walk_row(a.w, r);
        const int span = wr.span;
        const int nblk = (span + SC_BLK - 1) / SC_BLK;
        double evf[1], evb[1];
        walk_load<1>(wr.ek, M, lane, evf);
        walk_load<1, true>(wr.ek, M, lane, evb);
        // ---- rows of more than one block: x at the start of blocks 1 .. nblk - 1 ----
        if (nblk > 1) {
            SsFwdC<1> c;
            ss_load_fwd<1>(sa, lane, c);
            double x[1];
            walk_load_norm<1>(wr.ap, M, lane, x);
            walk_checkpoints<1, SC_BLK>(x, ckpt, nblk, lane, [&](const double (&u)[1], double (&out)[1], double &S) {
                pt_fwd_addends<1>(c, sa.c0, u, S, [&](int, double s0, double s1, double s2) { out[0] = evf[0] * (s0 + s1 + s2); });
            });
        }
        // ---- the blocks, last to first: y carried in a running scale across them ----
        double h[1];
        walk_load_norm<1, true>(a.w.beta + wr.row * a.w.Mp, M, lane, h);
        // column `st` of sum_p x_{p-1}(i) w_p(st) / Z_p.  A PLAIN fp64 sum, on purpose: every term is a product of probabilities, none
        // negative, so n positions leave it within n 2^-53 of its value and 64 compensation registers per lane buy nothing.  A change
        // that makes the terms signed (a tangent of x or w in here) has to compensate it, as g below and pt_add's other users are.
        double O[64];
#pragma unroll
        for (int i = 0; i < 64; ++i) O[i] = 0.0;
        double g = 0.0, gc = 0.0;                                // sum_p gamma_p(st), compensated
        for (int b = nblk - 1; b >= 0; --b) {
            const int len = min(SC_BLK, span - b * SC_BLK);
            {
                // forward through the block: x_{p-1} and T^T x_{p-1} of every position p of the block, parked as floats
                SsFwdC<1> c;
                ss_load_fwd<1>(sa, lane, c);
                double x[1];
                walk_block_start<1>(wr.ap, ckpt, b, M, lane, x);
                for (int t = 0; t < len; ++t) {
                    double out[1], tx = 0.0, S;
                    pt_fwd_addends<1>(c, sa.c0, x, S, [&](int, double s0, double s1, double s2) { tx = s0 + s1 + s2; });
                    px[t * 64 + lane] = (float)x[0];
                    ptx[t * 64 + lane] = (float)tx;
                    out[0] = evf[0] * tx;
                    walk_rescale<1>(x, out, (float)S);
                }
            }
            // the parked vectors are read back by OTHER lanes of this wavefront: the LDS stores have to be done first (a wavefront's
            // LDS operations complete in order; the fence keeps the compiler from moving a load above them)
            __threadfence_block();
            {
                SsBwdC<1> c;
                ss_load_bwd<1>(sa, lane, c);
                for (int t = len - 1; t >= 0; --t) {
                    const double w = evb[0] * h[0];
                    const double txv = (double)ptx[t * 64 + st];
                    const double Z = wave_sum_dpp(txv * w);
                    const double q = w / Z;                      // w_p(st) / Z_p
                    pt_add(g, gc, txv * q);                      // gamma_p(st)
                    const float4 *xr = reinterpret_cast<const float4 *>(px + t * 64);
#pragma unroll
                    for (int i4 = 0; i4 < 16; ++i4) {
                        const float4 v = xr[i4];                 // (the same address in every lane: a broadcast)
                        O[4 * i4 + 0] = __builtin_fma((double)v.x, q, O[4 * i4 + 0]);
                        O[4 * i4 + 1] = __builtin_fma((double)v.y, q, O[4 * i4 + 1]);
                        O[4 * i4 + 2] = __builtin_fma((double)v.z, q, O[4 * i4 + 2]);
                        O[4 * i4 + 3] = __builtin_fma((double)v.w, q, O[4 * i4 + 3]);
                    }
                    if (t > 0 || b > 0) {
                        double out[1];
                        float Sw;
                        ss_bwd_step<1>(c, h, evb, out, Sw);
                        walk_rescale<1>(h, out, Sw);
                    }
                }
            }
            // (the next block's forward walk overwrites what this block's backward walk has just read: LDS operations of one
            // wavefront complete in order, and the fence keeps the compiler from moving a store above the loads)
            __threadfence_block();
        }
        // ---- the contraction: one reduction per direction and part, the states in the wavefront's fixed order ----
        const double gs = g + gc;
        const double *ge = a.GE + (size_t)wr.kid * nder * 64 + st;
        for (int d = 0; d < nder; ++d) {
            const double *tb = a.dT + (size_t)d * 64 * 64 + st;
            double p = 0.0;
#pragma unroll
            for (int i = 0; i < 64; ++i) p = __builtin_fma(O[i], tb[i * 64], p);
            const double tr = wave_sum_dpp(p);
            const double em = wave_sum_dpp(gs * ge[(size_t)d * 64]);
            if (lane < 3) a.out[((size_t)lane * nder + d) * LD + r] = lane == 0 ? 0.0 : lane == 1 ? em : tr;
        }
    }
}

// Column j of the selection = caller's row l = start + j step: the sum of its pieces first[l] .. first[l + 1] - 1 (ascending, one
// thread per direction and column; first == nullptr: no row was cut, the piece is the row).  eng [3][nder][Le + 1] ->
// parts != 0: out [3][nder][ncols];  parts == 0: out [nder][ncols] = (initial + emission) + transition.
__global__ __launch_bounds__(256) void k_score_select(PostSel sel, long long Le, int nder, int parts, const int *__restrict__ first,
                                                      const double *__restrict__ eng, double *__restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= sel.ncols * nder) return;
    const long long d = idx / sel.ncols, j = idx - d * sel.ncols;
    const long long l = sel.start + j * sel.step;
    const long long p0 = first ? first[l] : l, p1 = first ? first[l + 1] : l + 1;
    double v[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const double *src = eng + ((size_t)x * nder + d) * (Le + 1);
        double s = 0.0, c = 0.0;
        for (long long p = p0; p < p1; ++p) pt_add(s, c, src[p]);
        v[x] = s + c;
        if (parts) out[((size_t)x * nder + d) * sel.ncols + j] = v[x];
    }
    if (!parts) out[(size_t)d * sel.ncols + j] = (v[0] + v[1]) + v[2];
}

// P [L + 1]: prefix positions of the caller's rows.  out[d][w] = sum_l overlap(l, w) / s_l * v[d][l], rows ascending; column 0 (its
// initial part) goes to window 0, in front of the rows.  One wavefront per window, as k_post_transition_windows: bisection in P,
// then lane d adds up direction d.  v [nder][L + 1] (all caller's rows), nder <= 64.
__global__ __launch_bounds__(256) void k_score_windows(long long L, long long W, long long nwin, int nder, const long long *__restrict__ P,
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
    if (lane >= nder) return;
    const double *src = v + (size_t)lane * (L + 1);
    double s = 0.0, c = 0.0;
    if (w == 0) pt_add(s, c, src[0]);
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
