// simulate_dev.hpp - draws of (hidden path, observations) from the model itself: the forward process whose marginal likelihood the
// E-step computes ("Simulation").  Included from engine.hip behind the posterior headers (pp_uniform, ss_scan, dpp0 and
// lane_get come from there); the host side is smcpp_simulate in engine_products.hpp, the contract is in include/smcpp_engine.h.
//
// Positions 0 .. N; x_0 ~ pi, x_p ~ T(x_{p-1}, .), o_p ~ Ebar(. | x_p) over the caller's alphabet.  The walk is by EVENTS: from
// (p, i) a geometric number G of quiet positions (state kept, quiet key emitted; P(G >= g) = s_i^g, s_i = T(i, i) Ebar(q | i)) is
// skipped with one uniform, then the successor state at p + G + 1 is drawn with weights T(i, j), j != i, and T(i, i)(1 - Ebar(q | i)),
// then its key with weights E[k][j] (the quiet key's weight 0 where the state stayed).  Both draws are inverse CDFs in ASCENDING
// order, x = min{ j : C_j > u C_last }, clamped to the last index - the rule of posterior_paths_dev.hpp.
//
//   k_simulate            one persistent wavefront per (contig, replicate); lanes over the states (state lane NPL + k) and over the
//                         alphabet entries (chunks of 64); the CDF is the lane-local prefix plus the DPP wave scan, the hit a ballot
//
// What depends on the state alone - log s_i and the weight of staying loud - comes from the host in fp64 (SimArgs::ls, ::wst); the
// kernel reads row i of T densely, so any T works.  No LDS, no atomics, no waiting on another wavefront; every loop bound is a kernel
// argument: at most `cap` events per replicate and call, after which the replicate's (event, position, state) is written out and a
// later call resumes from it with the same bits.
#pragma once

namespace smcpp_dev {

struct SimArgs {
    int M, MS, A, q;            // states, padded states (64 NPL), alphabet entries, the quiet entry's index IN the alphabet
    const double *T;            // [M][MS] row-major, zero beyond state M - 1
    const double *EA;           // [M][A]: E[alphabet entry k][state m] at [m][k]
    const double *ls;           // [M] log s_i (-inf: s_i = 0; >= 0: s_i >= 1, the run never ends)
    const double *wst;          // [M] T(i, i) (1 - Ebar(q | i))
    const double *pi;           // [MS], zero beyond state M - 1
    const long long *len;       // [contigs] N
    unsigned k0, k1;            // Philox key
    unsigned contig0;           // counter word 3 of contig 0 of the call
    long long rep0, nreps;      // replicates rep0 .. rep0 + nreps - 1 (counter word 2)
    long long units;            // contigs x nreps
    long long cap;              // events per replicate and call
    const long long *resume_in; // [units][3] (event, position, state; state -1: x_0 not drawn yet) or nullptr: all from the start
    int *x0;                    // [units] the state at position 0 where this call drew it, else -1
    long long *nev;             // [units] loud positions written by this call
    long long *pos;             // [units][cap]
    int *state, *key;           // [units][cap]
    long long *resume_out;      // [units][3]
};

// inverse CDF over the lane's NPL ascending entries w[]: the first index whose inclusive sum exceeds u times the total
template <int NPL>
__device__ __forceinline__ int sim_draw(const double (&w)[NPL], double u, int last, double c15, double c31) {
    double lp[NPL];
    lp[0] = w[0];
#pragma unroll
    for (int k = 1; k < NPL; ++k) lp[k] = lp[k - 1] + w[k];
    const double incl = ss_scan(lp[NPL - 1], c15, c31);
    const double ex = dpp0<DPP_WSHR1>(incl);                               // the lanes below (lane 0: 0)
    const double thr = u * lane_get(ex + lp[NPL - 1], 63);
    int below = 0;                                                         // entries of this lane with C <= thr (C ascends in the lane)
#pragma unroll
    for (int k = 0; k < NPL; ++k) below += (ex + lp[k] > thr) ? 0 : 1;
    const unsigned long long hit = __builtin_amdgcn_ballot_w64(below < NPL);
    if (hit == 0ull) return last;
    const int fl = (int)__builtin_ctzll(hit);
    return min(fl * NPL + __builtin_amdgcn_readlane(below, fl), last);
}

// weight of alphabet entry c0 + lane in state j (skip: the entry that weighs nothing, or -1)
__device__ __forceinline__ double sim_key_w(const double *__restrict__ ea, int A, int idx, int skip) {
    const bool live = idx < A && idx != skip;
    return live ? ea[live ? idx : 0] : 0.0;
}

template <int NPL>
__global__ __launch_bounds__(256) void k_simulate(SimArgs a, int nwaves) {
    constexpr int MS = 64 * NPL;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nwaves) return;
    const int M = a.M, A = a.A;
    const double c15 = ((lane >> 4) & 1) ? 1.0 : 0.0, c31 = ((lane >> 4) >= 2) ? 1.0 : 0.0;
    for (long long un = gw; un < a.units; un += nwaves) {
        const long long c = un / a.nreps;
        const unsigned rep = (unsigned)(a.rep0 + (un - c * a.nreps)), ctg = a.contig0 + (unsigned)c;
        const long long N = a.len[c];
        long long e = 0, p = 0;
        int i = -1;
        if (a.resume_in) { e = a.resume_in[3 * un]; p = a.resume_in[3 * un + 1]; i = (int)a.resume_in[3 * un + 2]; }
        i = ss_uni(i);
        int x0 = -1;
        if (i < 0) {
            // x_0 ~ pi: the spare uniform t = 3 of event 0
            double w[NPL];
#pragma unroll
            for (int k = 0; k < NPL; ++k) w[k] = a.pi[lane * NPL + k];
            i = ss_uni(sim_draw<NPL>(w, pp_uniform(a.k0, a.k1, 3, rep, ctg), M - 1, c15, c31));
            x0 = i;
        }
        long long cnt = 0;
        const size_t o = (size_t)un * (size_t)a.cap;
        while (p < N && cnt < a.cap) {
            // ---- u_0: the quiet run ----
            const double u0 = pp_uniform(a.k0, a.k1, 4 * e, rep, ctg);
            const double lsi = a.ls[i];
            const long long room = N - p;
            long long G = room;
            if (lsi < 0.0) {
                const double r = floor(log(1.0 - u0) / lsi);               // (1 - u_0 is exact; s_i = 0: -x / -inf = 0)
                G = r >= (double)room ? room : (long long)r;
            }
            if (G >= room) { ++e; p = N; break; }                          // the contig ends inside the run
            p += G + 1;
            // ---- u_1: the successor state at position p ----
            const double *tr = a.T + (size_t)i * MS + lane * NPL;
            const double wi = a.wst[i];
            double w[NPL];
#pragma unroll
            for (int k = 0; k < NPL; ++k) w[k] = (lane * NPL + k == i) ? wi : tr[k];
            const int j = ss_uni(sim_draw<NPL>(w, pp_uniform(a.k0, a.k1, 4 * e + 1, rep, ctg), M - 1, c15, c31));
            // ---- u_2: the key at position p, the alphabet in chunks of 64 entries ----
            const double u2 = pp_uniform(a.k0, a.k1, 4 * e + 2, rep, ctg);
            const double *ea = a.EA + (size_t)j * A;
            const int skip = j == i ? a.q : -1;
            double tot = 0.0;
            for (int c0 = 0; c0 < A; c0 += 64) tot += lane_get(ss_scan(sim_key_w(ea, A, c0 + lane, skip), c15, c31), 63);
            const double thr = u2 * tot;
            double carry = 0.0;
            int kx = A - 1;
            for (int c0 = 0; c0 < A; c0 += 64) {
                const double incl = ss_scan(sim_key_w(ea, A, c0 + lane, skip), c15, c31);
                const unsigned long long hit = __builtin_amdgcn_ballot_w64(c0 + lane < A && carry + incl > thr);
                if (hit != 0ull) { kx = c0 + (int)__builtin_ctzll(hit); break; }
                carry += lane_get(incl, 63);
            }
            if (lane == 0) { a.pos[o + cnt] = p; a.state[o + cnt] = j; a.key[o + cnt] = kx; }
            i = j;
            ++e; ++cnt;
        }
        if (lane == 0) {
            a.x0[un] = x0;
            a.nev[un] = cnt;
            a.resume_out[3 * un] = e; a.resume_out[3 * un + 1] = p; a.resume_out[3 * un + 2] = i;
        }
    }
}

}  // namespace smcpp_dev
