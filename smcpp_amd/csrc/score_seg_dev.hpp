// score_seg_dev.hpp - EXACT windows of the score track ("Score track": exact windows): on an engine row that a window
// boundary cuts strictly inside, every window gets the score of the positions that actually lie in it, not the row's total
// apportioned over its base pairs.  Included from engine.hip behind score_vec_dev.hpp (SvArgs, SV_BLK, sv_bwd_step) and
// loglik_track_dev.hpp (LlItem, ll_uni, ll_row_of); the host side is in engine_products.hpp (smcpp_score_windows_exact).  The vector
// form only: M <= 256, one to four states per lane.
//
//   k_score_segments_vec<NPL>   one persistent wavefront per ITEM of a host-built table (LlItem, ascending positions): an engine row
//                               with at least one window boundary STRICTLY inside it.  [3][nder][slots]: an item with nq boundaries
//                               owns the nq + 1 consecutive slots from its `seg` on, in ascending window order
//   k_score_windows_exact       [nder][n_windows]: whole engine rows from k_score_rows_vec's output, cut ones from the slots; one
//                               wavefront per window, lane d adds up direction d
//
// The walk is k_score_rows_vec's, statement by statement: blocks of at most 64 positions, fp64 checkpoints at the block starts of
// longer rows, forward from the stored float alpha with four parked floats per position and state, backward from the stored beta with
// one reduction per position into the five accumulators.  What differs is the sink.  Position p >= 1 of the contig lies in window
// (p - 1) / W, so the position at in-row offset o (1 .. span) is the FIRST of its window when o - 1 is the offset of a boundary,
// first - q0 + k W.  The backward loop runs over the positions descending; when it has added such a position - a wave-uniform test on
// the item's fields, no per-position table - it contracts the accumulators with the planes and G_E per direction as the row's end
// does in k_score_rows_vec (pt_add, two wavefront reductions per direction), writes the segment's slot and zeroes them.  The row's
// first position closes the last open segment.
// Every sum runs in a fixed order; no atomics; every loop bound is a kernel argument or an entry of the table; a value does not
// depend on the launch shape, the number of wavefronts or what ran before.
#pragma once

namespace smcpp_dev {

struct SgArgs {
    SvArgs v;                   // the rows, the tables and the wavefronts' scratch (v.L and v.out are not used here)
    int nitems;
    const LlItem *items;        // [nitems] q0 = the position in front of the row, first = its first boundary, nq boundaries
    long long W;                // the window width: boundary k of an item is first + k W
    long long nslots;           // slots of all items
    double *seg;                // [3][nder][nslots]: initial (zero), emission, transition
};

template <int NPL>
__global__ __launch_bounds__(256) void k_score_segments_vec(SsArgs sa, SgArgs g, int nwaves) {
    constexpr int MS = 64 * NPL;
    const SvArgs &a = g.v;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const int M = a.M, Mp = a.Mp, nder = a.nder;
    const size_t LD = (size_t)g.nslots;
    float *park = a.park + (size_t)gw * SV_BLK * 4 * MS;
    double *ckpt = a.ckpt + (size_t)gw * a.nck * MS;
    for (int it = gw; it < g.nitems; it += nwaves) {
        const LlItem item = g.items[it];
        const int r = ss_uni(item.row), nq = ss_uni(item.nq);
        const long long seg = ll_uni(item.seg);
        const size_t row = (size_t)(a.base + r);
        const int kid = ss_uni(a.rowinfo[row].kid), gid = ss_uni(a.rowinfo[row].gid);
        const int span = gid < 0 ? 1 : ss_uni(a.g_span[gid]);
        const double *ek = a.E + (size_t)kid * Mp;
        const float *ap = a.alpha + (row - 1) * Mp;
        const double *bp = a.beta + row * Mp;
        const int nblk = (span + SV_BLK - 1) / SV_BLK;
        // the segment that is open (the last one: the backward walk closes them descending) and the in-row offset of the boundary in
        // front of it; with kq == 0 no boundary is left and the row's first position closes the segment
        int kq = nq;
        long long nb = ll_uni(item.first) - ll_uni(item.q0) + (long long)(nq - 1) * g.W;
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
        // the four shares and g at state st[k] of the OPEN segment: plain fp64 sums of products of probabilities, none negative
        double aD[NPL], aL[NPL], aU1[NPL], aU2[NPL], aG[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) aD[k] = aL[k] = aU1[k] = aU2[k] = aG[k] = 0.0;
        const double *ge = a.GE + (size_t)kid * nder * MS + lane * NPL;
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
                    // ---- the flush: this position (in-row offset o) is the first of its window, or of the row ----
                    const int o = b * SV_BLK + t + 1;
                    const bool first_of_row = o == 1;
                    if (first_of_row || (kq > 0 && (long long)(o - 1) == nb)) {
                        const int slot = first_of_row ? 0 : kq;                         // (a table that fits the row: kq == 0 at o == 1)
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
                            if (lane < 3) g.seg[((size_t)lane * nder + d) * LD + (size_t)(seg + slot)] = lane == 0 ? 0.0 : lane == 1 ? em : tr;
                        }
#pragma unroll
                        for (int k = 0; k < NPL; ++k) aD[k] = aL[k] = aU1[k] = aU2[k] = aG[k] = 0.0;
                        kq = slot - 1;
                        nb -= g.W;
                    }
                }
            }
            // (the next block's forward walk overwrites what this block's backward walk has just read: the fence keeps the compiler
            // from moving a store above the loads, and every load has delivered its value - the sums depend on them)
            __threadfence_block();
        }
    }
}

// EP [Le + 1]: the position prefix of the ENGINE's rows; eng [3][nder][Le + 1]: k_score_rows_vec's output; it / nit: the item table
// the segments were walked by (ascending q0); seg [3][nder][nslots].  Window w = base pairs [w W, (w + 1) W): the engine rows that
// overlap it ascending - a row wholly inside adds its total (initial + emission) + transition, a cut one its item's slot for this
// window, seg + (w - the item's first window q0 / W) -, compensated.  Column 0 (its initial part) goes to window 0, in front of the rows.
__global__ __launch_bounds__(256) void k_score_windows_exact(long long Le, long long W, long long nwin, int nder,
                                                             const long long *__restrict__ EP, const double *__restrict__ eng,
                                                             const LlItem *__restrict__ it, int nit, long long nslots,
                                                             const double *__restrict__ seg, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nwin) return;
    const long long total = EP[Le];
    const long long lo = w * W, hi = min(lo + W, total);
    long long a = 1, b = Le;                                    // first engine row i >= 1 with EP[i] > lo (it exists: lo < EP[Le])
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (EP[mid] > lo) b = mid; else a = mid + 1;
    }
    if (lane >= nder) return;
    const size_t LD = (size_t)Le + 1;
    const double *e0 = eng + (size_t)lane * LD, *e1 = eng + ((size_t)nder + lane) * LD, *e2 = eng + ((size_t)2 * nder + lane) * LD;
    const double *s0 = seg + (size_t)lane * nslots, *s1 = seg + ((size_t)nder + lane) * nslots, *s2 = seg + ((size_t)2 * nder + lane) * nslots;
    double s = 0.0, c = 0.0;
    if (w == 0) pt_add(s, c, (e0[0] + e1[0]) + e2[0]);
    long long p0 = EP[a - 1];
    for (long long i = a; i <= Le && p0 < hi; ++i) {
        const long long p1 = EP[i];
        if (p0 >= lo && p1 <= hi) {
            pt_add(s, c, (e0[i] + e1[i]) + e2[i]);
        } else {
            int x = 0, y = nit - 1;                              // the item of row i: the one with q0 == p0
            while (x < y) {
                const int mid = (x + y) >> 1;
                if (it[mid].q0 >= p0) y = mid; else x = mid + 1;
            }
            const long long k = nit > 0 && it[x].q0 == p0 ? w - p0 / W : -1;
            if (k < 0 || k > it[x].nq) {
                pt_add(s, c, __builtin_nan(""));                 // (a table that does not hold the row: never an address)
            } else {
                const long long u = it[x].seg + k;
                pt_add(s, c, (s0[u] + s1[u]) + s2[u]);
            }
        }
        p0 = p1;
    }
    out[(size_t)lane * nwin + w] = s + c;
}

}  // namespace smcpp_dev
