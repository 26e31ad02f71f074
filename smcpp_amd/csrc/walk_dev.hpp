// walk_dev.hpp - what the product kernels that walk an engine row over the stored vectors of an E-step share ("the
// walk's leaves"): the rows they walk (WalkRows, walk_row), the lane layout (walk_load, walk_load_norm), the rescaling of a step, the
// fp64 checkpoints of a row of more than one block, and the compensated sum.  Included from engine.hip behind chains_ss.hpp (ss_uni,
// wave_sum_dpp) and in front of the product files.  Every kernel keeps its own loops over rows, blocks and positions, its own parking
// layout and its own sink; nothing here calls back into one.
//
// The lane layout: a wavefront holds 64 NPL states, NPL consecutive ones per lane.  The forward walk holds state lane NPL + k in
// entry k of the lane, the backward walk holds the states REVERSED, as the backward generators are stored.  States from M
// on are padding: they load as zero, from a clamped address.
#pragma once

namespace smcpp_dev {

// s += v with the rounding error of the addition kept in c (Neumaier's form of Kahan's sum; the total is s + c)
__device__ __forceinline__ void pt_add(double &s, double &c, double v) {
    const double t = s + v;
    c += (fabs(s) >= fabs(v)) ? (s - t) + v : (v - t) + s;
    s = t;
}

// The rows a walk reads: what the E-step stored, and the row table that says which key and span a row has.
struct WalkRows {
    int M, Mp;
    long long base;             // global row of the contig's row 0
    const RowInfo *rowinfo;     // [global rows] {key id, group id or -1}
    const int *g_span;          // [groups]
    const double *E;            // [K][Mp]
    const float *alpha;         // [global rows][Mp] stored forward vectors (row r: at the END of row r)
    const double *beta;         // [global rows][Mp] stored backward vectors (row r: at the END of row r); null for a forward-only walk
};

// Engine row r of the contig (wave uniform): its emission vector and the stored forward vector in front of it.  (The stored backward
// vector at its end, beta + row Mp, is formed by the walks that have one: WalkRows::beta is null in a forward-only walk.)
struct WalkRow {
    size_t row;                 // global row
    int kid, span;
    const double *ek;
    const float *ap;
};
__device__ __forceinline__ WalkRow walk_row(const WalkRows &w, int r) {
    WalkRow h;
    h.row = (size_t)(w.base + r);
    h.kid = ss_uni(w.rowinfo[h.row].kid);
    const int gid = ss_uni(w.rowinfo[h.row].gid);
    h.span = gid < 0 ? 1 : ss_uni(w.g_span[gid]);
    h.ek = w.E + (size_t)h.kid * w.Mp;
    h.ap = w.alpha + (h.row - 1) * w.Mp;
    return h;
}

// v = p in the forward (REV = false: entry k of a lane is state lane NPL + k) or the reversed layout (state 64 NPL - 1 - that),
// widened to double; a padding state loads as zero, from a clamped address (nothing beyond p[M - 1] is read).  The mask is spelled
// out here, not behind a helper of its own, on purpose: through one, k_post_transitions<4> passes 168 registers and loses its third
// wavefront per SIMD.  That is a property of one compiler's register allocation, not of the code: after a compiler change, compare
// -Rpass-analysis=kernel-resource-usage before folding anything here.
template <int NPL, bool REV = false, typename T>
__device__ __forceinline__ void walk_load(const T *p, int M, int lane, double (&v)[NPL]) {
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int st = REV ? 64 * NPL - 1 - (lane * NPL + k) : lane * NPL + k;
        const bool live = st < M;
        v[k] = live ? (double)p[live ? st : 0] : 0.0;
    }
}
// ... scaled to sum one over the wavefront (the sum is taken in the loading loop: two passes cost registers at four states per lane)
template <int NPL, bool REV = false, typename T>
__device__ __forceinline__ void walk_load_norm(const T *p, int M, int lane, double (&v)[NPL]) {
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const int st = REV ? 64 * NPL - 1 - (lane * NPL + k) : lane * NPL + k;
        const bool live = st < M;
        v[k] = live ? (double)p[live ? st : 0] : 0.0;
        part += v[k];
    }
    const double i0 = 1.0 / wave_sum_dpp(part);
#pragma unroll
    for (int k = 0; k < NPL; ++k) v[k] *= i0;
}

// x = out / S by the hardware's float reciprocal: a rescaling only, which whoever normalises a position cancels.  The factor is
// handed back for the walk that keeps its logarithm.
template <int NPL>
__device__ __forceinline__ double walk_rescale(double (&x)[NPL], const double (&out)[NPL], float S) {
    const double inv = (double)__builtin_amdgcn_rcpf(S);
#pragma unroll
    for (int k = 0; k < NPL; ++k) x[k] = out[k] * inv;
    return inv;
}

// The fp64 checkpoints of a row of more than one block, [blocks - 1][64 NPL] in the wavefront's own scratch: checkpoint b - 1 is x at
// the start of block b.  A lane reads back what it has written itself: program order, no fence.  The pass that fills them
// runs forward once from x at the row's start and keeps x at the start of blocks 1 .. nblk - 1 of BLK positions;
// step(x, out, S): one position, out = e o (T^T x), S = sum x.
template <int NPL, int BLK, typename Step>
__device__ __forceinline__ void walk_checkpoints(double (&x)[NPL], double *ckpt, int nblk, int lane, Step &&step) {
    for (int b = 1; b < nblk; ++b) {
        for (int t = 0; t < BLK; ++t) {
            double out[NPL], S;
            step(x, out, S);
            walk_rescale<NPL>(x, out, (float)S);
        }
#pragma unroll
        for (int k = 0; k < NPL; ++k) ckpt[(size_t)(b - 1) * (64 * NPL) + lane * NPL + k] = x[k];
    }
}
// x at the start of block b: the stored vector in front of the row, scaled to sum one, or checkpoint b - 1
template <int NPL>
__device__ __forceinline__ void walk_block_start(const float *ap, const double *ckpt, int b, int M, int lane, double (&x)[NPL]) {
    if (b == 0) {
        walk_load_norm<NPL>(ap, M, lane, x);
    } else {
#pragma unroll
        for (int k = 0; k < NPL; ++k) x[k] = ckpt[(size_t)(b - 1) * (64 * NPL) + lane * NPL + k];
    }
}

}  // namespace smcpp_dev
