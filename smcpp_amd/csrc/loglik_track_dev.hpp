// loglik_track_dev.hpp - the log-likelihood TRACK of the last E-step: l(p) = log P(o_1 .. o_p) per caller's row, per position of a
// grid and per window ("Log-likelihood track").  Included from engine.hip behind walk_dev.hpp (the leaves of the row
// walk) and posterior_pos_dev.hpp; the host side is in engine_products.hpp (smcpp_loglik_rows / _positions / _windows).
// Forward quantities only: the stored float alpha and log c of
// every engine row, which every E-step leaves behind - save_gamma is not needed, and the posterior buffers are not touched.
//
// Positions 0 .. N of a contig (0 = column 0; engine row r covers the `span` positions behind EP[r - 1], EP = the position prefix
// of the ENGINE's rows):
//     l(0) = 0,   l(EP[r]) = pre[r] = sum_{i <= r} log c_i,
//     inside row r (q = 1 .. span):  x_0 = the stored alpha in front of the row, normalised;  x_q ~ e o (T^T x_{q-1});
//     z_q = sum(e o T^T x_{q-1}) / sum(x_{q-1}),  A_q = sum_{t <= q} log z_t,   l(EP[r-1] + q) = pre[r-1] + log c_r  A_q / A_span.
//
//   k_ll_scan_partials / _of_partials / _down   pre[]: inclusive fp64 scan of log c over the engine rows of one contig, in a fixed
//                                 order (block sums, one block over the block sums, downsweep: the three launches of shaping.hpp)
//   k_ll_rows                     log c of the caller's rows of a selection: differences of pre[] at the caller's row ends
//   k_ll_ends                     the grid positions that are the END of an engine row (and position 0): straight from pre[]
//   k_ll_walk<NPL>                one persistent wavefront per ITEM of a host-built table (LlItem, ascending positions): an engine row
//                                 with at least one query position STRICTLY inside it.  Forward only: ss_fwd_step from the stored
//                                 alpha, x rescaled by rcpf of the running sum, the logs accumulated in fp64; A_q goes to the item's
//                                 slots of the output, and when the row's end is reached (A_span) the same wavefront turns them
//                                 into l.  Query t of an item is position first + t step: no per-position table
//   k_ll_windows                  out[w] = l(min((w + 1) W, N)) - l(w W): a boundary on a row end from pre[] (binary search in EP),
//                                 a boundary inside a row from the walk's output
//
// The sum of a step is not formed on its own: ss_fwd_step hands back S_{t-1} = sum(x_{t-1}) of its INPUT, x_t = out_t inv_t with
// inv_t = rcpf(S_{t-1}) (a float, so log(inv_t) is the log of the very number x was multiplied with), and
//     z_t = S_t / (inv_t S_{t-1})   =>   A_q = log S_q - log S_0 - sum_{t <= q} log inv_t.
// S_q is taken by wave_sum_dpp at the query positions and at the row's end only; it never feeds back into x, so A_q is a function
// of the stored vector and q alone.  No atomics, no waiting on another wavefront; every loop bound is a kernel argument or an entry
// of the host-built table.  A value does not depend on the grid, the launch shape, the number of wavefronts or what ran before.
#pragma once

namespace smcpp_dev {

constexpr int LL_SCAN_BLOCK = 256;

// ---- pre[i] = sum_{1 <= r <= i} v[r] (v = log c of the contig's engine rows, v[0] unused), pre[0] = 0; n = rows 1 .. n ----
__global__ __launch_bounds__(LL_SCAN_BLOCK) void k_ll_scan_partials(long long n, const double *__restrict__ v, double *__restrict__ partial) {
    __shared__ double red[LL_SCAN_BLOCK];
    const long long i = (long long)blockIdx.x * LL_SCAN_BLOCK + threadIdx.x + 1;
    red[threadIdx.x] = i <= n ? v[i] : 0.0;
    __syncthreads();
    for (int off = LL_SCAN_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
// one block: exclusive scan of the nb block sums in place (thread t owns `per` consecutive ones)
__global__ __launch_bounds__(LL_SCAN_BLOCK) void k_ll_scan_of_partials(long long nb, double *__restrict__ partial) {
    __shared__ double part[LL_SCAN_BLOCK];
    const long long per = (nb + LL_SCAN_BLOCK - 1) / LL_SCAN_BLOCK;
    const long long lo = (long long)threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    double s = 0.0;
    for (long long i = lo; i < hi; ++i) s += partial[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < LL_SCAN_BLOCK; off <<= 1) {        // Hillis-Steele inclusive scan of the thread sums
        const double u = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0.0;
        __syncthreads();
        part[threadIdx.x] += u;
        __syncthreads();
    }
    double run = threadIdx.x ? part[threadIdx.x - 1] : 0.0;
    for (long long i = lo; i < hi; ++i) { const double u = partial[i]; partial[i] = run; run += u; }
}
__global__ __launch_bounds__(LL_SCAN_BLOCK) void k_ll_scan_down(long long n, const double *__restrict__ v, const double *__restrict__ partial,
                                                               double *__restrict__ pre) {
    __shared__ double t[LL_SCAN_BLOCK];
    const long long i = (long long)blockIdx.x * LL_SCAN_BLOCK + threadIdx.x + 1;
    t[threadIdx.x] = i <= n ? v[i] : 0.0;
    __syncthreads();
    for (int off = 1; off < LL_SCAN_BLOCK; off <<= 1) {
        const double u = (int)threadIdx.x >= off ? t[threadIdx.x - off] : 0.0;
        __syncthreads();
        t[threadIdx.x] += u;
        __syncthreads();
    }
    if (i <= n) pre[i] = partial[blockIdx.x] + t[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 0) pre[0] = 0.0;
}

// log c of the caller's rows start, start + step, .. (ncols of them); first: piece_first_dev (nullptr: no row is cut).  Row 0 gives 0.
__global__ __launch_bounds__(256) void k_ll_rows(long long start, long long step, long long ncols, const int *__restrict__ first,
                                                 const double *__restrict__ pre, double *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncols) return;
    const long long l = start + j * step;
    if (l == 0) { out[j] = 0.0; return; }
    const long long e1 = first ? first[l + 1] - 1 : l, e0 = first ? first[l] - 1 : l - 1;
    out[j] = pre[e1] - pre[e0];
}

// first engine row i in 1 .. Le with EP[i] >= p (1 <= p <= EP[Le])
__device__ __forceinline__ long long ll_row_of(const long long *__restrict__ EP, long long Le, long long p) {
    long long a = 1, b = Le;
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (EP[mid] >= p) b = mid; else a = mid + 1;
    }
    return a;
}

// the grid positions that are position 0 or the end of an engine row; the others are the walk's
__global__ __launch_bounds__(256) void k_ll_ends(long long pos0, long long step, long long npos, long long Le,
                                                 const long long *__restrict__ EP, const double *__restrict__ pre, double *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= npos) return;
    const long long p = pos0 + j * step;
    if (p == 0) { out[j] = 0.0; return; }
    const long long i = ll_row_of(EP, Le, p);
    if (EP[i] == p) out[j] = pre[i];
}

struct LlItem {
    long long q0;               // the position in front of the row
    long long first;            // the row's first query position (q0 < first < q0 + span); query t is first + t step
    long long seg;              // the output slot of the first query
    int row;                    // engine row (>= 1)
    int nq;                     // queries strictly inside the row (>= 1)
};

struct LlArgs {
    WalkRows w;                 // (forward only: beta is null)
    int nitems;
    const double *logc;         // [global rows]
    const double *pre;          // [Le + 1] of this contig
    const LlItem *items;        // [nitems]
    long long step;             // distance of two query positions (the grid's step, the window width)
    double *out;                // the items' slots: A_q during the walk, l afterwards
    double *ratio;              // [nitems] |A_span / log c_r - 1|
};

__device__ __forceinline__ long long ll_uni(long long v) {
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((long long)hi << 32) | (unsigned int)lo;
}

template <int NPL>
__global__ __launch_bounds__(256) void k_ll_walk(SsArgs sa, LlArgs a, int nwaves) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const int M = a.w.M;
    SsFwdC<NPL> c;
    ss_load_fwd<NPL>(sa, lane, c);
    for (int it = gw; it < a.nitems; it += nwaves) {
        const LlItem item = a.items[it];
        const int r = ss_uni(item.row), nq = ss_uni(item.nq);
        const long long q0 = ll_uni(item.q0), seg = ll_uni(item.seg), first = ll_uni(item.first);
        const WalkRow wr = walk_row(a.w, r);
        const size_t row = wr.row;
        const int span = wr.span;
        double x[NPL], ev[NPL];
        walk_load_norm<NPL>(wr.ap, M, lane, x);                            // the plain stored vector (DESIGN.md says why)
        walk_load<NPL>(wr.ek, M, lane, ev);
        double acc = 0.0, As = 0.0;                                        // acc = - log S_0 - sum_t log inv_t
        long long qn = first - q0;                                         // the in-row offset of the next query
        int cnt = 0;
        for (int t = 1; t <= span; ++t) {
            double out[NPL], S;
            ss_fwd_step<NPL>(c, x, ev, out, S);
            acc -= log(walk_rescale<NPL>(x, out, (float)S));
            if (t == 1) acc -= log(S);
            double px = 0.0;
#pragma unroll
            for (int k = 0; k < NPL; ++k) px += x[k];
            const bool query = cnt < nq && (long long)t == qn;
            if (query || t == span) {
                const double A = log(wave_sum_dpp(px)) + acc;
                if (query) {
                    if (lane == 0) a.out[seg + cnt] = A;
                    ++cnt;
                    qn += a.step;
                }
                As = A;                                                    // (the last one stands: t == span)
            }
        }
        // the slots are read back by OTHER lanes of this wavefront: the stores have to be acknowledged first
        __threadfence_block();
        const double lc = a.logc[row], l0 = a.pre[r - 1];
        for (int u = lane; u < nq; u += 64) {
            const double A = a.out[seg + u];
            const double f = As != 0.0 ? A / As : (double)(first - q0 + (long long)u * a.step) / (double)span;
            a.out[seg + u] = l0 + lc * f;
        }
        if (lane == 0) a.ratio[it] = lc != 0.0 ? fabs(As / lc - 1.0) : fabs(As);
    }
}

// l(b) of a window boundary 0 <= b <= N: row ends from pre[], the others from the walk's slots (the item that holds b: the last
// one with q0 < b; its slot (b - first) / W)
__device__ __forceinline__ double ll_at(long long b, long long W, long long Le, const long long *__restrict__ EP,
                                        const double *__restrict__ pre, const LlItem *__restrict__ it, int nit,
                                        const double *__restrict__ bnd) {
    if (b == 0) return 0.0;
    const long long i = ll_row_of(EP, Le, b);
    if (EP[i] == b) return pre[i];
    int lo = 0, hi = nit - 1;                                              // (an item of row i exists: b lies strictly inside it)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (it[mid].q0 < b) lo = mid; else hi = mid - 1;
    }
    const long long t = nit > 0 && b >= it[lo].first ? (b - it[lo].first) / W : -1;
    if (t < 0 || t >= it[lo].nq) return __builtin_nan("");                 // (a table that does not hold b: never an address)
    return bnd[it[lo].seg + t];
}

__global__ __launch_bounds__(256) void k_ll_windows(long long W, long long nwin, long long Le, const long long *__restrict__ EP,
                                                    const double *__restrict__ pre, const LlItem *__restrict__ it, int nit,
                                                    const double *__restrict__ bnd, double *__restrict__ out) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwin) return;
    const long long N = EP[Le];
    const long long lo = w * W, hi = min(lo + W, N);
    out[w] = ll_at(hi, W, Le, EP, pre, it, nit, bnd) - ll_at(lo, W, Le, EP, pre, it, nit, bnd);
}

}  // namespace smcpp_dev
