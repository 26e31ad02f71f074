// posterior_paths_dev.hpp - joint draws of the hidden-state path from the posterior of the last save_gamma E-step, by forward
// filtering and backward sampling ("Posterior paths").  Included from engine.hip behind posterior_trans_dev.hpp (whose
// row walk - blocks of 64 positions, fp64 checkpoints of long rows - is repeated here BY HAND, not through the leaves of
// walk_dev.hpp: with them k_post_paths compiles to other code at every state count, 0.5 - 2.5 % slower where it was measured and
// with another scratch size at 16 states per lane; profiles/walk_leaves_refactor.log); the host side is in engine_products.hpp
// (smcpp_posterior_sample_rows / _sample_positions).
//
// Positions 0 .. N of a contig (0 = column 0, engine row r covers the `span` positions behind the end of row r - 1), forward vectors
// a_0 = the stored float alpha of column 0, a_p = e_p o (T^T a_{p-1}) advanced from the stored float alpha at the row's start by
// ss_fwd_step and parked as floats.  Path k:  x_N ~ a_N,  x_q | x_{q+1} = j ~ a_q(i) T(i, j),  every draw an inverse CDF over the
// states in ASCENDING order:  C_i = w_0 + .. + w_i,  x = min{ i : C_i > u C_{M-1} } (M - 1 if there is none), u from Philox4x32-10
// with key = the seed's two words and counter = (q lo, q hi, k, contig).  A draw therefore depends on the stored vectors, the seed,
// the contig, the path and the position - on nothing else: not on how paths are grouped, what a call returns or what ran before.
//
//   k_post_paths          one persistent wavefront per BATCH of paths: it walks the engine rows from the last to the first, a row in
//                         blocks of at most 64 positions (last block first); the forward walk of a block parks a_q once, then every
//                         path of the batch walks the block backwards against the same parked vectors
//   k_post_paths_select   the pieces of a caller's row merged (counts added, state of the last piece), a column selection taken
//
// One draw: the lane multiplies its parked a_q entries with row j of the transposed dense T (j is wave uniform; row M of that table is
// all ones: "no successor", the draw of x_N), takes a lane-local prefix and a DPP wave scan in fp64, compares with u times the total,
// and the first lane of the ballot names the state.  State lane NPL + k: ascending.  The lane reads back only what it parked itself.
// The state of a path between blocks (its x_{q+1}, the counts of the row it is in) lives in lane i of the wavefront for path i of the
// batch: at most 64 paths per batch.  No atomics, no waiting on another wavefront; every loop bound is a kernel argument.
#pragma once

namespace smcpp_dev {

struct PpArgs {
    int M, Mp, L;               // L: ENGINE rows of the contig (rows 1 .. L; row 0 is column 0)
    int nck;                    // checkpoint vectors per wavefront (blocks of the longest row - 1)
    long long base;             // global row of the contig's row 0
    const RowInfo *rowinfo;     // [global rows] {key id, group id or -1}
    const int *g_span;          // [groups]
    const double *E;            // [K][Mp]
    const float *alpha;         // [global rows][Mp] stored forward vectors (row r: at the END of row r)
    const double *TT;           // [M + 1][MS]: TT[j][i] = T(i, j), zero beyond state M - 1; row M: ones on the live states
    float *park;                // [wavefronts][64][MS]
    double *ckpt;               // [wavefronts][nck][MS]
    unsigned k0, k1;            // Philox key: the seed's low / high word
    unsigned contig;            // counter word 3
    long long path0, npaths;    // paths path0 .. path0 + npaths - 1
    long long nbatches;
    int batch;                  // paths per batch (1 .. 64)
    long long N;                // last position of the contig
    long long pos0, pos1;       // window of the per-position output
    int *pos_out;               // [npaths][pos1 - pos0] or nullptr
    int *rows_out;              // [3][npaths][L + 1] (state, up, down per ENGINE row) or nullptr
};

constexpr int PP_BLK = 64;

__device__ __forceinline__ unsigned pp_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

// Philox4x32-10 (Salmon et al., SC'11): output words 0 and 1 of counter (q lo, q hi, path, contig) as a double in [0, 1)
__device__ __forceinline__ double pp_uniform(unsigned k0, unsigned k1, long long q, unsigned path, unsigned contig) {
    unsigned c0 = (unsigned)((unsigned long long)q & 0xffffffffull), c1 = (unsigned)((unsigned long long)q >> 32), c2 = path, c3 = contig;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = pp_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = pp_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (double)(((unsigned long long)(c0 >> 5) << 26) + (unsigned long long)(c1 >> 6)) * 0x1p-53;
}

// One draw: weights pv[k] * tt[k] of the lane's states lane NPL + k -> the first state whose inclusive sum exceeds u times the total.
template <int NPL>
__device__ __forceinline__ int pp_draw(const float (&pv)[NPL], const double *__restrict__ tt, double u, int M, int lane, double c15,
                                       double c31) {
    double lp[NPL];
    lp[0] = (double)pv[0] * tt[0];
#pragma unroll
    for (int k = 1; k < NPL; ++k) lp[k] = __builtin_fma((double)pv[k], tt[k], lp[k - 1]);
    const double incl = ss_scan(lp[NPL - 1], c15, c31);
    const double ex = dpp0<DPP_WSHR1>(incl);                               // the lanes below (lane 0: 0)
    const double thr = u * lane_get(ex + lp[NPL - 1], 63);
    int below = 0;                                                         // states of this lane with C_i <= thr (C ascends in the lane)
#pragma unroll
    for (int k = 0; k < NPL; ++k) below += (ex + lp[k] > thr) ? 0 : 1;
    const unsigned long long hit = __builtin_amdgcn_ballot_w64(below < NPL);
    if (hit == 0ull) return M - 1;
    const int fl = (int)__builtin_ctzll(hit);
    return min(fl * NPL + __builtin_amdgcn_readlane(below, fl), M - 1);
}

template <int NPL>
__global__ __launch_bounds__(256) void k_post_paths(SsArgs sa, PpArgs a, int nwaves) {
    constexpr int MS = 64 * NPL;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const int M = a.M, Mp = a.Mp;
    const size_t LD = (size_t)a.L + 1;
    const long long W = a.pos1 - a.pos0;
    float *park = a.park + (size_t)gw * PP_BLK * MS;
    double *ckpt = a.ckpt + (size_t)gw * a.nck * MS;
    const double c15 = ((lane >> 4) & 1) ? 1.0 : 0.0, c31 = ((lane >> 4) >= 2) ? 1.0 : 0.0;
    const bool want_rows = a.rows_out != nullptr;
    for (long long bt = gw; bt < a.nbatches; bt += nwaves) {
        const long long pfirst = bt * a.batch;                             // first path of the batch, counted from path0
        const int nb = (int)min((long long)a.batch, a.npaths - pfirst);
        // lane i: path i of the batch - its x_{q+1} (M: none yet), the end state and the counts of the row position q + 1 lies in
        int pj = M, pes = 0, pup = 0, pdn = 0;
        long long q = a.N;                                                 // the last position of the row in hand
        bool stop = false;
        for (int r = a.L; r >= 1 && !stop; --r) {
            const size_t row = (size_t)(a.base + r);
            const int kid = ss_uni(a.rowinfo[row].kid), gid = ss_uni(a.rowinfo[row].gid);
            const int span = gid < 0 ? 1 : ss_uni(a.g_span[gid]);
            const long long q0 = q - span;                                 // the position in front of the row
            if (!want_rows && q < a.pos0) break;                           // nothing below is asked for
            const double *ek = a.E + (size_t)kid * Mp;
            const float *ap = a.alpha + (row - 1) * Mp;
            const int nblk = (span + PP_BLK - 1) / PP_BLK;
            // ---- rows of more than one block: a at the start of blocks 1 .. nblk - 1 ----
            if (nblk > 1) {
                SsFwdC<NPL> c;
                ss_load_fwd<NPL>(sa, lane, c);
                double ev[NPL];
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const int st = lane * NPL + k;
                    const bool live = st < M;
                    ev[k] = live ? ek[live ? st : 0] : 0.0;
                }
                double x[NPL], part = 0.0;
#pragma unroll
                for (int k = 0; k < NPL; ++k) {
                    const int st = lane * NPL + k;
                    const bool live = st < M;
                    x[k] = live ? (double)ap[live ? st : 0] : 0.0;
                    part += x[k];
                }
                const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
                for (int k = 0; k < NPL; ++k) x[k] *= i0;
                for (int b = 1; b < nblk; ++b) {
                    for (int t = 0; t < PP_BLK; ++t) {
                        double out[NPL], S;
                        ss_fwd_step<NPL>(c, x, ev, out, S);
                        const double inv = (double)__builtin_amdgcn_rcpf((float)S);        // (a rescaling only: a draw is scale free)
#pragma unroll
                        for (int k = 0; k < NPL; ++k) x[k] = out[k] * inv;
                    }
#pragma unroll
                    for (int k = 0; k < NPL; ++k) ckpt[(size_t)(b - 1) * MS + lane * NPL + k] = x[k];
                }
            }
            // ---- the blocks, last to first ----
            for (int b = nblk - 1; b >= 0; --b) {
                const int len = min(PP_BLK, span - b * PP_BLK);
                const long long qb = q0 + (long long)b * PP_BLK;           // block position t is contig position qb + t + 1
                if (!want_rows && qb + len < a.pos0) { stop = true; break; }
                {
                    // forward through the block: a_q of every position of the block, parked once for the whole batch
                    // (the generators are loaded inside the walk that uses them: sixteen states per lane do not keep them across the draws)
                    SsFwdC<NPL> c;
                    ss_load_fwd<NPL>(sa, lane, c);
                    double ev[NPL];
#pragma unroll
                    for (int k = 0; k < NPL; ++k) {
                        const int st = lane * NPL + k;
                        const bool live = st < M;
                        ev[k] = live ? ek[live ? st : 0] : 0.0;
                    }
                    double x[NPL];
                    if (b == 0) {
                        double part = 0.0;
#pragma unroll
                        for (int k = 0; k < NPL; ++k) {
                            const int st = lane * NPL + k;
                            const bool live = st < M;
                            x[k] = live ? (double)ap[live ? st : 0] : 0.0;
                            part += x[k];
                        }
                        const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
                        for (int k = 0; k < NPL; ++k) x[k] *= i0;
                    } else {
#pragma unroll
                        for (int k = 0; k < NPL; ++k) x[k] = ckpt[(size_t)(b - 1) * MS + lane * NPL + k];
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
                // (every lane reads back the entries it has parked itself: program order, no fence)
                const bool row_top = b == nblk - 1;
                for (int i = 0; i < nb; ++i) {
                    int j = __builtin_amdgcn_readlane(pj, i), es = __builtin_amdgcn_readlane(pes, i);
                    int up = __builtin_amdgcn_readlane(pup, i), dn = __builtin_amdgcn_readlane(pdn, i);
                    const long long prel = pfirst + i;
                    const unsigned path = (unsigned)(a.path0 + prel);
                    int xs = 0;                                            // lane t: the state at block position t
                    for (int t = len - 1; t >= 0; --t) {
                        const float *pk = park + (size_t)t * MS + lane * NPL;
                        float pv[NPL];
#pragma unroll
                        for (int k = 0; k < NPL; ++k) pv[k] = pk[k];
                        const double u = pp_uniform(a.k0, a.k1, qb + t + 1, path, a.contig);
                        const int x = pp_draw<NPL>(pv, a.TT + (size_t)j * MS + lane * NPL, u, M, lane, c15, c31);
                        if (j < M) { up += x < j ? 1 : 0; dn += x > j ? 1 : 0; }            // the transition INTO position qb + t + 2
                        if (row_top && t == len - 1) {
                            // the first draw of row r: row r + 1 is complete
                            if (want_rows && r < a.L && lane == 0) {
                                int *o = a.rows_out + (size_t)prel * LD + (r + 1);
                                o[0] = es; o[(size_t)a.npaths * LD] = up; o[2 * (size_t)a.npaths * LD] = dn;
                            }
                            es = x; up = 0; dn = 0;
                        }
                        if (lane == t) xs = x;
                        j = x;
                    }
                    if (lane == i) { pj = j; pes = es; pup = up; pdn = dn; }
                    if (a.pos_out) {
                        const long long p = qb + lane + 1;
                        if (lane < len && p >= a.pos0 && p < a.pos1) a.pos_out[(size_t)prel * W + (p - a.pos0)] = xs;
                    }
                }
            }
            q = q0;
        }
        if (stop || (!want_rows && a.pos0 > 0)) continue;
        // ---- column 0: a_0 is the stored vector itself ----
        float pv[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int st = lane * NPL + k;
            const bool live = st < M;
            pv[k] = live ? a.alpha[(size_t)a.base * Mp + (live ? st : 0)] : 0.f;
        }
        for (int i = 0; i < nb; ++i) {
            const int j = __builtin_amdgcn_readlane(pj, i), es = __builtin_amdgcn_readlane(pes, i);
            int up = __builtin_amdgcn_readlane(pup, i), dn = __builtin_amdgcn_readlane(pdn, i);
            const long long prel = pfirst + i;
            const double u = pp_uniform(a.k0, a.k1, 0, (unsigned)(a.path0 + prel), a.contig);
            const int x = pp_draw<NPL>(pv, a.TT + (size_t)j * MS + lane * NPL, u, M, lane, c15, c31);
            if (j < M) { up += x < j ? 1 : 0; dn += x > j ? 1 : 0; }
            if (lane == 0) {
                if (want_rows) {
                    int *o = a.rows_out + (size_t)prel * LD;
                    const size_t pl = (size_t)a.npaths * LD;
                    if (a.L >= 1) { o[1] = es; o[pl + 1] = up; o[2 * pl + 1] = dn; }
                    o[0] = x; o[pl] = 0; o[2 * pl] = 0;
                }
                if (a.pos_out && a.pos0 == 0) a.pos_out[(size_t)prel * W] = x;
            }
        }
    }
}

// Column j of the selection = caller's row l = start + j step of path p: its pieces first[l] .. first[l + 1] - 1 merged - the state of
// the last piece, the counts added (first == nullptr: no row was cut).  eng [3][npaths][Le + 1] -> out [3][npaths][ncols].
__global__ __launch_bounds__(256) void k_post_paths_select(PostSel sel, long long Le, long long npaths, const int *__restrict__ first,
                                                           const int *__restrict__ eng, int *__restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= npaths * sel.ncols) return;
    const long long p = idx / sel.ncols, j = idx - p * sel.ncols;
    const long long l = sel.start + j * sel.step;
    const long long p0 = first ? first[l] : l, p1 = first ? first[l + 1] : l + 1;
    const size_t plane = (size_t)npaths * (Le + 1);
    const int *src = eng + (size_t)p * (Le + 1);
    int up = 0, dn = 0;
    for (long long e = p0; e < p1; ++e) { up += src[plane + e]; dn += src[2 * plane + e]; }
    const size_t oplane = (size_t)npaths * sel.ncols;
    out[idx] = src[p1 - 1];
    out[oplane + idx] = up;
    out[2 * oplane + idx] = dn;
}

}  // namespace smcpp_dev
