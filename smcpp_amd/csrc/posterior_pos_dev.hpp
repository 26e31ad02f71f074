// posterior_pos_dev.hpp - per-POSITION posterior products of the last save_gamma E-step: the marginal gamma_p of single positions on a
// grid, its summaries, and the window averages that are exact on long rows ("Posterior positions").  Included from
// engine.hip behind walk_dev.hpp (pt_add), posterior_trans_dev.hpp (the row walk, repeated here BY HAND: with the leaves of walk_dev.hpp
// the scratch of k_post_positions at 16 states per lane moves by up to 50 %; profiles/walk_leaves_refactor.log) and
// posterior_paths_dev.hpp; the host side is in engine_products.hpp (smcpp_posterior_positions / _position_summary / _windows_exact).
//
// Positions 0 .. N of a contig (0 = column 0, engine row r covers the `span` positions behind the end of row r - 1):
//     a_0 = pi, a_p = e_p o (T^T a_{p-1}),   b_N = 1, b_{p-1} = T (e_p o b_p),   gamma_p(i) = a_p(i) b_p(i) / sum_m a_p(m) b_p(m).
//
//   k_post_positions<NPL, Sink>   one persistent wavefront per ITEM of a host-built table (PqItem, ascending positions).  An item is an
//                                 engine row to WALK - the walk of k_post_transitions with one parked vector instead of three - or a
//                                 position whose marginal is STORED: position 0 and the caller's rows of one position, whose marginal
//                                 is the per-row posterior every other product reports (rows[l] / colsum[l], bit for bit)
//   k_post_windows_exact          [M x n_windows]: rows inside one window from the stored per-row posterior, rows that a window boundary
//                                 cuts from the segment sums of the walk; one wavefront per (window, 64 states), ascending positions
//
// The walk: a row in blocks of at most 64 positions, last block first.  A row of more than one block first runs forward once and keeps
// x at every block start (fp64 checkpoints).  The forward walk of a block (ss_fwd_step from the stored float alpha at the row's start
// - pq_start: entries at the engine's 1e-10 floor are restored where the row in front is one position -, rescaled by rcpf of the running sum) parks a_p of every position as floats; the backward walk (ss_bwd_step from the stored beta at
// the row's end) multiplies the parked vector with h = b_p, normalises by the wavefront sum in fp64 and hands the position to the sink.
// h lives in REVERSED state order (lane, k hold state 64 NPL - 1 - (lane NPL + k)), and so does everything a sink sees.
// Scratch is global, not LDS: one layout for every NPL, 16 KB NPL per wavefront.  No atomics, no waiting on another wavefront; every
// loop bound is a kernel argument or an entry of the host-built table.  A value depends on the stored vectors and on the position
// alone: not on the grid, the launch shape or what ran before.
#pragma once

namespace smcpp_dev {

struct PqItem {
    long long end;              // the last position of the item (engine row r: the position at its end; stored: the position itself)
    int row;                    // engine row to walk (>= 1), unused for a stored item
    int src;                    // < 0: walk; >= 0: the caller's row whose stored posterior is the marginal (0: column 0)
    int seg;                    // segments sink: index of the item's first (lowest) segment
    int pad;
};

struct PqArgs {
    int M, Mp;
    int nck;                    // checkpoint vectors per wavefront (blocks of the longest WALKED row - 1)
    int nitems;
    long long base;             // global row of the contig's row 0
    const RowInfo *rowinfo;     // [global rows] {key id, group id or -1}
    const int *g_span;          // [groups]
    const double *E;            // [K][Mp]
    const float *alpha;         // [global rows][Mp] stored forward vectors (row r: at the END of row r)
    const double *beta;         // [global rows][Mp] stored backward vectors (row r: at the END of row r)
    const PqItem *items;        // [nitems]
    const double *rows, *g0;    // per-row posteriors of the CALLER's rows (posterior_dev.hpp) and their sums
    const double *colsum;       // [Lu + 1]
    float *park;                // [wavefronts][64][MS]
    double *ckpt;               // [wavefronts][nck][MS]
    long long pos0, pos1, step, npos;   // the grid (columns, summary)
    double *out;                // columns: [M x npos]
    const double *w;            // summary: weights [M] or nullptr
    PostLevels lv;
    int *argmax;                // [npos] or nullptr
    double *mean;               // [npos] or nullptr
    int *qstate;                // [nq x npos] or nullptr
    long long W;                // segments: window width
    double *seg;                // segments: [segments][MS], states in natural order
};

constexpr int PQ_BLK = 64;

struct PqColumns { static constexpr int kind = 0; };
struct PqSummary { static constexpr int kind = 1; };
struct PqSegments { static constexpr int kind = 2; };

// The sink of one grid position j: g[k] = gamma_p(st(k)) (reversed state order, zero on the padding states).
template <int NPL, typename Sink>
__device__ __forceinline__ void pq_emit(const PqArgs &a, long long j, const double (&g)[NPL], int lane, double c15, double c31) {
    const int M = a.M;
    const auto st = [lane](int k) { return 64 * NPL - 1 - (lane * NPL + k); };
    if (Sink::kind == 0) {
#pragma unroll
        for (int k = 0; k < NPL; ++k)
            if (st(k) < M) a.out[(size_t)st(k) * a.npos + j] = g[k];
        return;
    }
    constexpr int MS = 64 * NPL;
    if (a.argmax) {
        // the lowest state that attains the maximum: inside the lane the later k (a lower state) wins a tie, across the lanes the
        // highest lane that holds the maximum
        double bv = g[0];
        int bs = st(0);
#pragma unroll
        for (int k = 1; k < NPL; ++k)
            if (g[k] >= bv) { bv = g[k]; bs = st(k); }
        double mx = bv;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(bv == mx);
        const int fl = 63 - (int)__builtin_clzll(hit);                     // (hit != 0: the maximum is some lane's)
        const int s = __builtin_amdgcn_readlane(bs, fl);
        if (lane == 0) a.argmax[j] = min(s, M - 1);
    }
    if (a.w && a.mean) {
        double part = 0.0;
#pragma unroll
        for (int k = 0; k < NPL; ++k) part = __builtin_fma(st(k) < M ? a.w[st(k) < M ? st(k) : 0] : 0.0, g[k], part);
        const double mu = wave_sum_dpp(part);
        if (lane == 0) a.mean[j] = mu;
    }
    if (a.lv.nq > 0 && a.qstate) {
        // C(m) = sum_{i <= m} gamma(i) = total - sum_{i > m} gamma(i): the exclusive prefix in the reversed layout.  It does not grow
        // along (lane, k), so the entries with C >= q are the first n of them, and the lowest such state is MS - n.
        double lp[NPL];
        lp[0] = g[0];
#pragma unroll
        for (int k = 1; k < NPL; ++k) lp[k] = lp[k - 1] + g[k];
        const double incl = ss_scan(lp[NPL - 1], c15, c31);
        const double ex = dpp0<DPP_WSHR1>(incl);                           // the lanes below (lane 0: 0)
        const double total = lane_get(incl, 63);
        double C[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) C[k] = total - (ex + (k == 0 ? 0.0 : lp[k - 1 < 0 ? 0 : k - 1]));
#pragma unroll
        for (int qi = 0; qi < 8; ++qi) {
            if (qi < a.lv.nq) {
                const double q = a.lv.q[qi];
                int n = 0;
#pragma unroll
                for (int k = 0; k < NPL; ++k) n += (int)__builtin_popcountll(__builtin_amdgcn_ballot_w64(C[k] >= q));
                if (lane == 0) a.qstate[(size_t)qi * a.npos + j] = min(MS - n, M - 1);
            }
        }
    }
}

// The forward vector in front of engine row r (global row `row`), normalised to sum one: the stored float alpha of row r - 1.  The
// engine stores alpha floored at 1e-10 (the reference's rule), and an entry AT the floor has lost its value: behind a heterozygous
// site the most recent states hold 1e-11 and less, and where b_p is three orders of magnitude above the other states' there, the
// floor shows as 1e-7 in gamma_p while the state refills.  Where row r - 1 is ONE position, such entries are restored by redoing
// that position in fp64 from the stored vector of row r - 2 (never above what is stored); behind a longer row they stay as stored.
template <int NPL>
__device__ __forceinline__ void pq_start(const SsArgs &sa, const PqArgs &a, int lane, int r, size_t row, double (&x)[NPL]) {
    const int M = a.M, Mp = a.Mp;
    const float *ap = a.alpha + (row - 1) * Mp;
    double part = 0.0;
    bool low = false;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int s = lane * NPL + k;
        const bool live = s < M;
        const float v = live ? ap[live ? s : 0] : 0.f;
        low = low || (live && v <= 1e-10f);
        x[k] = (double)v;
        part += x[k];
    }
    const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
    for (int k = 0; k < NPL; ++k) x[k] *= i0;
    if (r < 2 || __builtin_amdgcn_ballot_w64(low) == 0ull) return;         // (wave uniform)
    const int kid1 = ss_uni(a.rowinfo[row - 1].kid), gid1 = ss_uni(a.rowinfo[row - 1].gid);
    if (gid1 >= 0 && ss_uni(a.g_span[gid1]) != 1) return;
    const double *e1 = a.E + (size_t)kid1 * Mp;
    const float *a2 = a.alpha + (row - 2) * Mp;
    SsFwdC<NPL> c;
    ss_load_fwd<NPL>(sa, lane, c);
    double y[NPL], ev[NPL], out[NPL], S, p2 = 0.0;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int s = lane * NPL + k;
        const bool live = s < M;
        y[k] = live ? (double)a2[live ? s : 0] : 0.0;
        ev[k] = live ? e1[live ? s : 0] : 0.0;
        p2 += y[k];
    }
    const double i2 = 1.0 / wave_sum_dpp(p2);
#pragma unroll
    for (int k = 0; k < NPL; ++k) y[k] *= i2;
    ss_fwd_step<NPL>(c, y, ev, out, S);
    double po = 0.0;
#pragma unroll
    for (int k = 0; k < NPL; ++k) po += out[k];
    const double io = 1.0 / wave_sum_dpp(po);
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int s = lane * NPL + k;
        const bool live = s < M;
        if (live && ap[live ? s : 0] <= 1e-10f) x[k] = fmin(out[k] * io, x[k]);
    }
}

template <int NPL, typename Sink>
__global__ __launch_bounds__(256) void k_post_positions(SsArgs sa, PqArgs a, int nwaves) {
    constexpr int MS = 64 * NPL;
    constexpr bool SEG = Sink::kind == 2;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const int M = a.M, Mp = a.Mp;
    float *park = a.park + (size_t)gw * PQ_BLK * MS;
    double *ckpt = a.ckpt + (size_t)gw * a.nck * MS;
    const double c15 = ((lane >> 4) & 1) ? 1.0 : 0.0, c31 = ((lane >> 4) >= 2) ? 1.0 : 0.0;
    const auto st = [lane](int k) { return MS - 1 - (lane * NPL + k); };      // the state of entry k in the reversed layout
    for (int it = gw; it < a.nitems; it += nwaves) {
        const PqItem item = a.items[it];
        const int src = ss_uni(item.src);
        if (src >= 0) {
            // ---- a stored marginal: the per-row posterior of a caller's row of one position, or column 0 ----
            if constexpr (SEG) continue;                                             // (the table of the segments sink holds no such item)
            const double *g_ = post_row(a.rows, a.g0, Mp, src);
            const double cs = a.colsum[src];
            double g[NPL];
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const bool live = st(k) < M;
                g[k] = live ? g_[live ? st(k) : 0] / cs : 0.0;
            }
            pq_emit<NPL, Sink>(a, (item.end - a.pos0) / a.step, g, lane, c15, c31);
            continue;
        }
        const int r = ss_uni(item.row);
        const size_t row = (size_t)(a.base + r);
        const int kid = ss_uni(a.rowinfo[row].kid), gid = ss_uni(a.rowinfo[row].gid);
        const int span = gid < 0 ? 1 : ss_uni(a.g_span[gid]);
        const long long q0 = item.end - span;                              // the position in front of the row
        const double *ek = a.E + (size_t)kid * Mp;
        const double *bp = a.beta + row * Mp;
        const int nblk = (span + PQ_BLK - 1) / PQ_BLK;
        // ---- rows of more than one block: a at the start of blocks 1 .. nblk - 1 ----
        if (nblk > 1) {
            SsFwdC<NPL> c;
            ss_load_fwd<NPL>(sa, lane, c);
            double x[NPL], ev[NPL];
            pq_start<NPL>(sa, a, lane, r, row, x);
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const int s = lane * NPL + k;
                const bool live = s < M;
                ev[k] = live ? ek[live ? s : 0] : 0.0;
            }
            for (int b = 1; b < nblk; ++b) {
                for (int t = 0; t < PQ_BLK; ++t) {
                    double out[NPL], S;
                    ss_fwd_step<NPL>(c, x, ev, out, S);
                    const double inv = (double)__builtin_amdgcn_rcpf((float)S);            // (a rescaling only: it cancels)
#pragma unroll
                    for (int k = 0; k < NPL; ++k) x[k] = out[k] * inv;
                }
#pragma unroll
                for (int k = 0; k < NPL; ++k) ckpt[(size_t)(b - 1) * MS + lane * NPL + k] = x[k];
            }
        }
        // ---- the blocks, last to first: h = b_p carried in a running scale across them ----
        double h[NPL];
        {
            double part = 0.0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const bool live = st(k) < M;
                h[k] = live ? bp[live ? st(k) : 0] : 0.0;
                part += h[k];
            }
            const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
            for (int k = 0; k < NPL; ++k) h[k] *= i0;
        }
        // segments: sum of gamma_p between window boundaries (base pair b = position b + 1: window w starts at position w W + 1)
        double acc[SEG ? NPL : 1], cmp[SEG ? NPL : 1];
        long long wfirst = 0, sg = 0;
        if constexpr (SEG) {
#pragma unroll
            for (int k = 0; k < NPL; ++k) { acc[k] = 0.0; cmp[k] = 0.0; }
            wfirst = ((item.end - 1) / a.W) * a.W + 1;                     // the first position of the window the row ends in
            sg = item.seg + ((item.end - 1) / a.W - q0 / a.W);             // the row's last segment
        }
        bool stop = false;
        for (int b = nblk - 1; b >= 0 && !stop; --b) {
            const int len = min(PQ_BLK, span - b * PQ_BLK);
            const long long qb = q0 + (long long)b * PQ_BLK;               // block position t is contig position qb + t + 1
            if (!SEG && qb + len < a.pos0) break;                          // nothing of this block or below is asked for
            {
                // forward through the block: a_p of every position of the block, parked as floats
                SsFwdC<NPL> c;
                ss_load_fwd<NPL>(sa, lane, c);
                double x[NPL], ev[NPL];
                if (b == 0) {
                    pq_start<NPL>(sa, a, lane, r, row, x);                 // (the same bits as the checkpoint pass started from)
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
                    ss_fwd_step<NPL>(c, x, ev, out, S);
                    const double inv = (double)__builtin_amdgcn_rcpf((float)S);
                    float *pk = park + (size_t)t * MS + lane * NPL;
#pragma unroll
                    for (int k = 0; k < NPL; ++k) {
                        x[k] = out[k] * inv;
                        pk[k] = (float)x[k];
                    }
                }
            }
            // As in k_post_transitions: the parked vectors are read back by OTHER lanes of this wavefront (reversed state order), so
            // the stores have to be acknowledged first (one CU, one vector L1: a workgroup-scope fence is a wait, no cache maintenance)
            __threadfence_block();
            {
                SsBwdC<NPL> c;
                ss_load_bwd<NPL>(sa, lane, c);
                double ev[NPL];
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const bool live = st(k) < M;
                    ev[k] = live ? ek[live ? st(k) : 0] : 0.0;
                }
                for (int t = len - 1; t >= 0; --t) {
                    const long long p = qb + t + 1;
                    if (!SEG && p < a.pos0) { stop = true; break; }        // nothing below is asked for
                    const float *pk = park + (size_t)t * MS;
                    bool want = true;
                    long long j = 0;
                    if (!SEG) {
                        want = p < a.pos1;
                        if (want) {
                            j = (p - a.pos0) / a.step;
                            want = a.pos0 + j * a.step == p;
                        }
                    }
                    if (want) {
                        double g[NPL], part = 0.0;
#pragma unroll
                        for (int k = 0; k < NPL; ++k) {
                            g[k] = st(k) < M ? (double)pk[st(k)] * h[k] : 0.0;
                            part += g[k];
                        }
                        const double iz = 1.0 / wave_sum_dpp(part);
#pragma unroll
                        for (int k = 0; k < NPL; ++k) g[k] *= iz;
                        if constexpr (SEG) {
#pragma unroll
                            for (int k = 0; k < NPL; ++k) pt_add(acc[k], cmp[k], g[k]);
                            if (p == wfirst || p == q0 + 1) {
                                // the segment is complete: positions max(wfirst, q0 + 1) .. of this window
#pragma unroll
                                for (int k = 0; k < NPL; ++k) {
                                    a.seg[(size_t)sg * MS + st(k)] = acc[k] + cmp[k];
                                    acc[k] = 0.0; cmp[k] = 0.0;
                                }
                                --sg;
                                wfirst -= a.W;
                            }
                        } else {
                            pq_emit<NPL, Sink>(a, j, g, lane, c15, c31);
                        }
                    }
                    if (t > 0 || b > 0) {
                        double out[NPL];
                        float Sw;
                        ss_bwd_step<NPL>(c, h, ev, out, Sw);
                        const double is = (double)__builtin_amdgcn_rcpf(Sw);          // (a rescaling only)
#pragma unroll
                        for (int k = 0; k < NPL; ++k) h[k] = out[k] * is;
                    }
                }
            }
            // (as in k_post_transitions: the next block's forward walk overwrites the scratch this block's backward walk has just
            // read; every load above has delivered its value - the sums depend on them - before the wavefront gets there)
        }
    }
}

// Exact window averages.  P [L + 1]: prefix positions of the caller's rows; row l covers base pairs [P[l-1], P[l]), window w covers
// [w W, min((w + 1) W, P[L])).  A row inside the window adds s_l rows[l] / colsum[l] (the stored posterior, as k_post_windows); a row
// that a boundary of the window cuts adds the segments of its walked engine rows that lie in the window: item i (it [nit], ascending)
// covers base pairs [it.end - span, it.end) and its segment in window w is it.seg + (w - first window of the item).  One wavefront per
// (window, 64 states), lane = state; the terms are added in ascending position order with a compensated sum.
__global__ __launch_bounds__(256) void k_post_windows_exact(int M, int Mp, int MS, long long L, long long W, long long nwin,
                                                            const long long *__restrict__ P, const double *__restrict__ rows,
                                                            const double *__restrict__ colsum, const PqItem *__restrict__ it,
                                                            const long long *__restrict__ it_start, int nit,
                                                            const double *__restrict__ seg, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nwin) return;
    const int m = blockIdx.y * 64 + lane;
    const bool live = m < M;
    const long long total = P[L];
    const long long lo = w * W, hi = min(lo + W, total);
    long long a = 1, b = L;                                     // first row l >= 1 with P[l] > lo (it exists: lo < P[L])
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (P[mid] > lo) b = mid; else a = mid + 1;
    }
    double s = 0.0, c = 0.0;
    long long p0 = P[a - 1];
    for (long long l = a; l <= L && p0 < hi; ++l) {
        const long long p1 = P[l];
        if (p0 >= lo && p1 <= hi) {
            if (live) pt_add(s, c, (double)(p1 - p0) * (rows[(size_t)l * Mp + m] / colsum[l]));
        } else {
            // the walked items of this row that reach into the window: the first item with end > max(p0, lo)
            const long long from = max(p0, lo), to = min(p1, hi);
            int ia = 0, ib = nit;
            while (ia < ib) {
                const int mid = (ia + ib) >> 1;
                if (it[mid].end > from) ib = mid; else ia = mid + 1;
            }
            for (int i = ia; i < nit && it_start[i] < to; ++i) {
                const long long sgi = it[i].seg + (w - it_start[i] / W);
                if (live) pt_add(s, c, seg[(size_t)sgi * MS + m]);
            }
        }
        p0 = p1;
    }
    if (live) out[(size_t)m * nwin + w] = (s + c) / (double)(hi - lo);
}

}  // namespace smcpp_dev
