// score_vec_dev.hpp - the VECTOR form of the score track's row walk ("Score track"): the transition part of a row without
// the M x M object of score_track_dev.hpp, at one to four states per lane (M <= 256).  Included from engine.hip behind
// score_track_dev.hpp (ScArgs' conventions, k_score_select / k_score_windows, which read this kernel's output unchanged); the host
// side is in engine_products.hpp (smcpp_im::score_rows_vec), the coefficient planes in engine_params.hpp (score_planes).
//
// T and its Jacobian are semiseparable (prep.hpp: TransitionGenJac): below the diagonal dT_d(i, j) / T(i, j) depends on the column
// only (cL_d(j)), above it dT_d(i, j) = (T(i, j) - c0) (cP_d(i) + cW_d(j)), the diagonal has cD_d(j).  So
//     sum_ij O(i, j) dT_d(i, j) = sum_j D(j) cD_d(j) + L(j) cL_d(j) + U1(j) cW_d(j) + U2(j) cP_d(j)
// with four M-vectors per row that do not depend on d.  With w_p = e o y_p and the addends of the forward scan step (pt_fwd_parts):
//     D(j)  = sum_p  d_j x_{p-1}(j)               w_p(j) / Z_p        the mass that stays
//     L(j)  = sum_p  g_j sum_{i>j} x_{p-1}(i)     w_p(j) / Z_p        the mass that arrives from above
//     U1(j) = sum_p  Z_j(x_{p-1})                 w_p(j) / Z_p        the Phi' part of the mass that arrives from below
//     U2(i) = sum_p  x_{p-1}(i) b_i V_i(w_p) / Z_p                    the same mass, by the state it leaves (the backward step's Phi' part)
// and g(j) = sum_p gamma_p(j) for the emission part.  x_{p-1}(i) is the parked stay addend over d_i: the host folds 1 / d_i into cP.
//
//   k_score_rows_vec<NPL>   one wavefront per ENGINE row: [3][nder][L + 1], the layout of k_score_rows
//
// The walk is k_post_transitions<NPL>'s, repeated BY HAND (with the leaves of walk_dev.hpp the kernel was 1.5 % slower on long un-binned
// rows; profiles/walk_leaves_refactor.log): blocks of at most 64 positions, fp64 checkpoints of x at the block starts of longer rows,
// forward from the stored float alpha, backward from the stored beta, rescaled at every step.  The forward walk of a block parks four
// floats per position and state in the wavefront's own global scratch (stay | from above | c0 part | Phi' part of the addend from
// below; Z_p and gamma_p come from the same floats, so a position's gamma sums to one); the backward walk reduces Z_p - ONE wavefront
// reduction per position - and adds the four shares and g into 5 NPL registers per lane.  It takes the backward step at EVERY
// position, a row's first included: U2 needs its Phi' part there.
// Every term is a product of probabilities, none negative: plain fp64 sums (score_track_dev.hpp argues the same for O).  The
// contraction, once per row, meets signed coefficients and is compensated (pt_add) before the wavefront reduction.  Every sum runs
// in a fixed order; no atomics; a value does not depend on the launch shape or on what ran before.
#pragma once

namespace smcpp_dev {

struct SvArgs {
    int M, Mp, L;               // L: ENGINE rows of the contig (rows 1 .. L; row 0 is column 0)
    int nck;                    // checkpoint vectors per wavefront (blocks of the longest row - 1)
    int nder;                   // directions
    long long base;             // global row of the contig's row 0
    const RowInfo *rowinfo;     // [global rows] {key id, group id or -1}
    const int *g_span;          // [groups]
    const double *E;            // [K][Mp]
    const float *alpha;         // [global rows][Mp] stored forward vectors (row r: at the END of row r)
    const double *beta;         // [global rows][Mp] stored backward vectors (row r: at the END of row r)
    const double *gamma0;       // [Mp] the contig's column 0 as stored (proportional to gamma_0)
    // MS = 64 NPL doubles per plane, zero beyond M.  The planes the backward walk's accumulators meet are stored by BACKWARD position
    // (state j at MS - 1 - j), as the backward generators are
    const double *Gpi;          // [nder][MS]      dpi_d / pi, state order
    const double *planes;       // [nder][4][MS]   cD | cL | cW | cP / d, mirrored
    const double *GE;           // [K][nder][MS]   dE_d[k] / E[k], mirrored
    float *park;                // [wavefronts][SV_BLK][4][MS]
    double *ckpt;               // [wavefronts][nck][MS]
    double *out;                // [3][nder][L + 1]: initial, emission, transition
};

constexpr int SV_BLK = 64;                                       // positions per block

// One position of the backward chain on w = e o y (ss_bwd_step's scans, chains_ss.hpp, at any NPL): out = T w, Sw = sum w (float
// accuracy), and bV[k] = b V, the Phi' part of out - what the states above receive through the upper triangle without the uniform mix.
template <int NPL>
__device__ __forceinline__ void sv_bwd_step(const SsBwdC<NPL> &c, const double (&w)[NPL], double (&out)[NPL], float &Sw, double (&bV)[NPL]) {
    double lg[NPL], u[NPL];
    float lf[NPL];
    lg[0] = c.g[0] * w[0];
    u[0] = w[0];
    lf[0] = (float)w[0];
#pragma unroll
    for (int k = 1; k < NPL; ++k) {
        lg[k] = __builtin_fma(c.g[k], w[k], lg[k - 1]);
        u[k] = __builtin_fma(c.a[k], u[k - 1], w[k]);
        lf[k] = lf[k - 1] + (float)w[k];
    }
    double p_ = lg[NPL - 1], z_ = u[NPL - 1];
    float f_ = lf[NPL - 1];
    {
        double tp, tz;
        float tf;
        tp = dpp0<DPP_SHR1>(p_); tz = dpp0<DPP_SHR1>(z_); tf = dpp0<DPP_SHR1>(f_); p_ += tp; z_ = __builtin_fma(c.lv[0], tz, z_); f_ += tf;
        tp = dpp0<DPP_SHR2>(p_); tz = dpp0<DPP_SHR2>(z_); tf = dpp0<DPP_SHR2>(f_); p_ += tp; z_ = __builtin_fma(c.lv[1], tz, z_); f_ += tf;
        tp = dpp0<DPP_SHR4>(p_); tz = dpp0<DPP_SHR4>(z_); tf = dpp0<DPP_SHR4>(f_); p_ += tp; z_ = __builtin_fma(c.lv[2], tz, z_); f_ += tf;
        tp = dpp0<DPP_SHR8>(p_); tz = dpp0<DPP_SHR8>(z_); tf = dpp0<DPP_SHR8>(f_); p_ += tp; z_ = __builtin_fma(c.lv[3], tz, z_); f_ += tf;
        tp = dpp0<DPP_BC15>(p_); tz = dpp0<DPP_BC15>(z_); tf = dpp0<DPP_BC15>(f_);
        p_ = __builtin_fma(c.c15, tp, p_); z_ = __builtin_fma(c.lv[4], tz, z_); f_ = __builtin_fmaf(c.c15f, tf, f_);
        tp = dpp0<DPP_BC31>(p_); tz = dpp0<DPP_BC31>(z_); tf = dpp0<DPP_BC31>(f_);
        p_ = __builtin_fma(c.c31, tp, p_); z_ = __builtin_fma(c.lv[5], tz, z_); f_ = __builtin_fmaf(c.c31f, tf, f_);
    }
    const double Gtot = lane_get(p_, 63);
    Sw = lane_get(f_, 63);
    const double LIp = dpp0<DPP_WSHR1>(z_);
    const double lexg = p_ - lg[NPL - 1];
    const float lexf = f_ - lf[NPL - 1];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const double inclG = lexg + lg[k];
        const double inclW = (double)(lexf + lf[k]);
        const double V = (k == 0) ? LIp : __builtin_fma(c.cumA[k - 1 < 0 ? 0 : k - 1], LIp, u[k - 1 < 0 ? 0 : k - 1]);
        bV[k] = c.b[k] * V;
        out[k] = __builtin_fma(c.dc[k], w[k], (Gtot - inclG) + __builtin_fma(c.c0, inclW, bV[k]));
    }
}

template <int NPL>
__global__ __launch_bounds__(256) void k_score_rows_vec(SsArgs sa, SvArgs a, int nwaves) {
    constexpr int MS = 64 * NPL;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const int M = a.M, Mp = a.Mp, nder = a.nder;
    const size_t LD = (size_t)a.L + 1;
    float *park = a.park + (size_t)gw * SV_BLK * 4 * MS;
    double *ckpt = a.ckpt + (size_t)gw * a.nck * MS;
    if (gw == 0) {
        // column 0: the initial part alone, from the stored column 0 normalised here (k_score_rows has the why)
        double g0[NPL], part = 0.0;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int st = lane * NPL + k;
            const bool live = st < M;
            g0[k] = live ? a.gamma0[live ? st : 0] : 0.0;
            part += g0[k];
        }
        const double i0 = 1.0 / wave_sum_dpp(part);
        for (int d = 0; d < nder; ++d) {
            const double *gp = a.Gpi + (size_t)d * MS + lane * NPL;
            double s = 0.0, sc = 0.0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) pt_add(s, sc, (g0[k] * i0) * gp[k]);
            const double v = wave_sum_dpp(s + sc);
            if (lane < 3) a.out[((size_t)lane * nder + d) * LD] = lane == 0 ? v : 0.0;
        }
    }
    for (int r = 1 + gw; r <= a.L; r += nwaves) {
        const size_t row = (size_t)(a.base + r);
        const int kid = ss_uni(a.rowinfo[row].kid), gid = ss_uni(a.rowinfo[row].gid);
        const int span = gid < 0 ? 1 : ss_uni(a.g_span[gid]);
        const double *ek = a.E + (size_t)kid * Mp;
        const float *ap = a.alpha + (row - 1) * Mp;
        const double *bp = a.beta + row * Mp;
        const int nblk = (span + SV_BLK - 1) / SV_BLK;
        // ---- rows of more than one block: x at the start of blocks 1 .. nblk - 1 ----
        if (nblk > 1) {
            SsFwdC<NPL> c;
            ss_load_fwd<NPL>(sa, lane, c);
            double x[NPL], ev[NPL], part = 0.0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const int st = lane * NPL + k;
                const bool live = st < M;
                x[k] = live ? (double)ap[live ? st : 0] : 0.0;
                ev[k] = live ? ek[live ? st : 0] : 0.0;
                part += x[k];
            }
            const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
            for (int k = 0; k < NPL; ++k) x[k] *= i0;
            for (int b = 1; b < nblk; ++b) {
                for (int t = 0; t < SV_BLK; ++t) {
                    double out[NPL], S;
                    pt_fwd_addends<NPL>(c, sa.c0, x, S, [&](int k, double s0, double s1, double s2) { out[k] = ev[k] * (s0 + s1 + s2); });
                    const double inv = (double)__builtin_amdgcn_rcpf((float)S);            // (a rescaling only: it cancels)
#pragma unroll
                    for (int k = 0; k < NPL; ++k) x[k] = out[k] * inv;
                }
#pragma unroll
                for (int k = 0; k < NPL; ++k) ckpt[(size_t)(b - 1) * MS + lane * NPL + k] = x[k];   // (read back by the lane that wrote it)
            }
        }
        // ---- the blocks, last to first: y carried in a running scale across them ----
        double h[NPL], evb[NPL];
        int st[NPL];
        {
            double part = 0.0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                st[k] = MS - 1 - (lane * NPL + k);
                const bool live = st[k] < M;
                h[k] = live ? bp[live ? st[k] : 0] : 0.0;
                evb[k] = live ? ek[live ? st[k] : 0] : 0.0;
                part += h[k];
            }
            const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
            for (int k = 0; k < NPL; ++k) h[k] *= i0;
        }
        // the four shares and g at state st[k]: PLAIN fp64 sums of terms that are products of probabilities, none negative
        double aD[NPL], aL[NPL], aU1[NPL], aU2[NPL], aG[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) aD[k] = aL[k] = aU1[k] = aU2[k] = aG[k] = 0.0;
        for (int b = nblk - 1; b >= 0; --b) {
            const int len = min(SV_BLK, span - b * SV_BLK);
            {
                // forward through the block: the addends of x_{p-1} of every position p of the block, parked as floats
                SsFwdC<NPL> c;
                ss_load_fwd<NPL>(sa, lane, c);
                double x[NPL], ev[NPL];
                if (b == 0) {
                    double part = 0.0;
#pragma unroll
                    for (int k = 0; k < NPL; ++k) {
                        const int s = lane * NPL + k;
                        const bool live = s < M;
                        x[k] = live ? (double)ap[live ? s : 0] : 0.0;
                        part += x[k];
                    }
                    const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
                    for (int k = 0; k < NPL; ++k) x[k] *= i0;
                } else {
#pragma unroll
                    for (int k = 0; k < NPL; ++k) x[k] = ckpt[(size_t)(b - 1) * MS + lane * NPL + k];
                }
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const int s = lane * NPL + k;
                    const bool live = s < M;
                    ev[k] = live ? ek[live ? s : 0] : 0.0;
                }
                for (int t = 0; t < len; ++t) {
                    double out[NPL], S;
                    float *pk = park + (size_t)t * 4 * MS + lane * NPL;
                    pt_fwd_parts<NPL>(c, x, S, [&](int k, double s0, double s1, double low, double Z) {
                        const double s2 = sa.c0 * low;
                        pk[k] = (float)s0; pk[MS + k] = (float)s1; pk[2 * MS + k] = (float)s2; pk[3 * MS + k] = (float)Z;
                        out[k] = ev[k] * (s0 + s1 + (s2 + Z));
                    });
                    const double inv = (double)__builtin_amdgcn_rcpf((float)S);
#pragma unroll
                    for (int k = 0; k < NPL; ++k) x[k] = out[k] * inv;
                }
            }
            // the parked addends are read back by OTHER lanes of this wavefront (reversed state order): the stores have to be
            // acknowledged first (one CU, one vector L1: a workgroup-scope fence is a wait, no cache maintenance)
            __threadfence_block();
            {
                SsBwdC<NPL> c;
                ss_load_bwd<NPL>(sa, lane, c);
                for (int t = len - 1; t >= 0; --t) {
                    const float *pk = park + (size_t)t * 4 * MS;
                    double w[NPL], f0[NPL], f1[NPL], fz[NPL], tx[NPL], zp = 0.0;
#pragma unroll
                    for (int k = 0; k < NPL; ++k) {
                        w[k] = evb[k] * h[k];
                        f0[k] = (double)pk[st[k]];
                        f1[k] = (double)pk[MS + st[k]];
                        fz[k] = (double)pk[3 * MS + st[k]];
                        tx[k] = (f0[k] + f1[k]) + ((double)pk[2 * MS + st[k]] + fz[k]);
                        zp = __builtin_fma(tx[k], w[k], zp);
                    }
                    const double iz = 1.0 / wave_sum_dpp(zp);                          // 1 / Z_p: the one reduction of the position
                    double out[NPL], bV[NPL];
                    float Sw;
                    sv_bwd_step<NPL>(c, w, out, Sw, bV);
#pragma unroll
                    for (int k = 0; k < NPL; ++k) {
                        const double q = w[k] * iz;                                     // w_p(st) / Z_p
                        aD[k] = __builtin_fma(f0[k], q, aD[k]);
                        aL[k] = __builtin_fma(f1[k], q, aL[k]);
                        aU1[k] = __builtin_fma(fz[k], q, aU1[k]);
                        aG[k] = __builtin_fma(tx[k], q, aG[k]);                         // gamma_p(st)
                        aU2[k] = __builtin_fma(f0[k] * iz, bV[k], aU2[k]);              // d x_{p-1}(st) b V / Z_p
                    }
                    if (t > 0 || b > 0) {
                        const double is = (double)__builtin_amdgcn_rcpf(Sw);           // (a rescaling only)
#pragma unroll
                        for (int k = 0; k < NPL; ++k) h[k] = out[k] * is;
                    }
                }
            }
            // (the next block's forward walk overwrites what this block's backward walk has just read: the fence keeps the compiler
            // from moving a store above the loads, and every load has delivered its value - the sums depend on them)
            __threadfence_block();
        }
        // ---- the contraction: one fused pass over the five planes per direction, one reduction per part ----
        const double *ge = a.GE + (size_t)kid * nder * MS + lane * NPL;
        for (int d = 0; d < nder; ++d) {
            const double *pl = a.planes + (size_t)d * 4 * MS + lane * NPL;
            double s = 0.0, sc = 0.0, e = 0.0, ec = 0.0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                pt_add(s, sc, aD[k] * pl[k]);
                pt_add(s, sc, aL[k] * pl[MS + k]);
                pt_add(s, sc, aU1[k] * pl[2 * MS + k]);
                pt_add(s, sc, aU2[k] * pl[3 * MS + k]);
                pt_add(e, ec, aG[k] * ge[(size_t)d * MS + k]);
            }
            const double tr = wave_sum_dpp(s + sc);
            const double em = wave_sum_dpp(e + ec);
            if (lane < 3) a.out[((size_t)lane * nder + d) * LD + r] = lane == 0 ? 0.0 : lane == 1 ? em : tr;
        }
    }
}

}  // namespace smcpp_dev
