// engine_products.hpp - part of the ONE translation unit engine.hip (included there, in order; not a standalone header):
// the host side of the products that read the stored vectors of an E-step - posterior columns, summaries and windows, transitions,
// paths, positions, the log-likelihood track, the score track - and of the simulation: argument checks, item tables, scratch sizing,
// launches, and their entry points of include/smcpp_engine.h.  The kernels are in the *_dev.hpp file each section names.

// The caller's rows of contig c with the pieces of every cut row added up, on the device ([Lu + 1][Mp]; row 0 is left to the caller).
const double *smcpp_im::merged_gamma(int c) {
    const int Lu = user_Ls[c];
    const int *first = piece_first_dev(c);
    d_gamma_user.alloc((size_t)(Lu + 1) * Mp);
    hipLaunchKernelGGL(k_gamma_merge, dim3((unsigned)ceil_div((long long)Lu * Mp, 256)), dim3(256), 0, stream, Mp, Lu,
                       first, (const double *)(d_gamma_rows.p + (size_t)contig_base[c] * Mp), d_gamma_user.p);
    return d_gamma_user.p;
}

// first[l] = the first piece (engine row) of caller's row l of contig c, first[Lu + 1] = one past the last piece; built on first use.
const int *smcpp_im::piece_first_dev(int c) {
    if (!split_spans) return nullptr;
    const int Lu = user_Ls[c];
    if (d_piece_first.size() != (size_t)n_contigs) d_piece_first.resize(n_contigs);
    if (!d_piece_first[c].p) {
        std::vector<int> first((size_t)Lu + 2, 0);
        const std::vector<int> &pr = piece_row[c];                 // piece -> caller's row (non-decreasing)
        for (int l = (int)pr.size() - 1; l >= 1; --l) first[pr[l]] = l;
        first[Lu + 1] = Ls[c] + 1;
        d_piece_first[c].upload(first, stream);
        HIPCHK(hipStreamSynchronize(stream));          // (`first` is a local: the copy has to be done before it goes)
    }
    return d_piece_first[c].p;
}

// ---- what the product calls share: the host side of a walk over the stored vectors of an E-step, the argument checks ----
// A fresh SsArgs on the generators of the last E-step's T: ss_gen uploaded on `stream`, M and Mp set.
SsArgs smcpp_im::walk_generators() {
    d_walk_gen.upload(ss_gen, stream);                 // (ss_gen is a member: it outlives the copy)
    SsArgs sa = SsArgs();
    sa.M = M; sa.Mp = Mp;
    set_generators(sa, d_walk_gen.p, 64 * NPL, ss_c0);
    return sa;
}

// The rows a walk over contig c reads: the stored vectors of the last E-step and its row table (walk_dev.hpp).
WalkRows smcpp_im::walk_rows(int c) {
    WalkRows w;
    w.M = M; w.Mp = Mp; w.base = contig_base[c];
    w.rowinfo = d_rowinfo.p; w.g_span = d_g_span.p; w.E = d_E.p; w.alpha = d_alpha.p; w.beta = d_beta.p;
    return w;
}

// The longest engine row of contig c (1: it has none), and the fp64 checkpoints a walk in blocks of `blk` positions keeps of such a row.
int smcpp_im::longest_row(int c) {
    int smax = 1;
    for (int i = 1; i <= Ls[c]; ++i) {
        const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
        if (ri.gid >= 0) smax = std::max(smax, groups[ri.gid].span);
    }
    return smax;
}
static int walk_checkpoints(int smax, int blk) { return (smax + blk - 1) / blk - 1; }

// Persistent wavefronts of a walk: one per unit of work up to `slots`, fewer where `per_wave` bytes of scratch each would pass
// `budget` in all (per_wave == 0: no scratch), at least one.
long long smcpp_im::walk_slots() const { return NPL >= 8 ? 1024 : 4096; }
static int walk_waves(long long units, long long slots, size_t per_wave, size_t budget = (size_t)1 << 30) {
    long long nw = std::min(units, slots);
    if (per_wave) nw = std::min(nw, (long long)(budget / per_wave));
    return (int)std::max<long long>(1, nw);
}

// f(std::integral_constant<int, x>()) for x = npl, the states per lane the walk kernels are instantiated at.
template <class F>
static void for_npl(int npl, F &&f) {
    switch (npl) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 8: f(std::integral_constant<int, 8>()); break;
        default: f(std::integral_constant<int, 16>());
    }
}

// The position prefix of the caller's rows of contig c on the device ([Lu + 1]), uploaded on first use.
const long long *smcpp_im::user_prefix_dev(int c) {
    if (d_user_prefix.size() != (size_t)n_contigs) d_user_prefix.resize(n_contigs);
    if (!d_user_prefix[c].p) {
        d_user_prefix[c].upload(user_prefix[c], stream);               // (a member: it outlives the copy)
        HIPCHK(hipStreamSynchronize(stream));
    }
    return d_user_prefix[c].p;
}

// ceil(P_L / window_bp), the windows of contig c, written to *n_windows where given; `who` opens the refusal of a window_bp below 1.
static long long window_count(smcpp_im *im, int c, long long window_bp, const char *who, long long *n_windows) {
    if (window_bp < 1) throw std::runtime_error(std::string(who) + ": window_bp < 1");
    const long long nwin = (im->user_prefix[c][im->user_Ls[c]] + window_bp - 1) / window_bp;
    if (n_windows) *n_windows = nwin;
    return nwin;
}

// pos0 / pos1 / step of a grid (`noun`: what an empty one is called) over the positions 0 .. P_L of contig c -> its positions
static long long check_position_grid(smcpp_im *im, const char *who, const char *noun, int c, long long pos0, long long pos1,
                                     long long step = 1) {
    const std::string w = std::string(who) + ": ";
    const long long N = im->user_prefix[c][im->user_Ls[c]];
    if (pos0 < 0) throw std::runtime_error(w + "pos0 < 0");
    if (pos1 > N + 1) throw std::runtime_error(w + "pos1 > P_L + 1 (the contig has " + std::to_string(N + 1) + " positions)");
    if (pos0 >= pos1) throw std::runtime_error(w + "empty " + noun + " (pos0 >= pos1)");
    if (step < 1) throw std::runtime_error(w + "step < 1");
    return (pos1 - pos0 + step - 1) / step;
}

// The quantile levels and the weights of a summary call.
static PostLevels check_levels(const char *who, int nq, const double *q) {
    PostLevels lv;
    lv.nq = 0;
    for (int k = 0; k < 8; ++k) lv.q[k] = 2.0;
    if (nq < 0 || nq > 8) throw std::runtime_error(std::string(who) + ": between 0 and 8 quantile levels");
    if (nq > 0 && !q) throw std::runtime_error(std::string(who) + ": quantile levels are missing");
    for (int k = 0; k < nq; ++k) {
        if (!(q[k] > 0.0 && q[k] < 1.0)) throw std::runtime_error(std::string(who) + ": a quantile level must lie in (0, 1)");
        lv.q[k] = q[k];
    }
    lv.nq = nq;
    return lv;
}
static void check_weights(const char *who, const double *weights, int M) {
    if (weights)
        for (int i = 0; i < M; ++i)
            if (!std::isfinite(weights[i])) throw std::runtime_error(std::string(who) + ": weight " + std::to_string(i) + " is not finite");
}

// ---- posterior products (posterior_dev.hpp) ----
static void post_need_gamma(smcpp_im *im, int c) {
    if (!im->estep_done) throw std::runtime_error("posterior products: no E-step has been run on this manager yet");
    if (!im->gamma_valid) throw std::runtime_error("posterior products: save_gamma was not set for the last E-step");
    if (c < 0 || c >= im->n_contigs) throw std::runtime_error("contig index out of range");
}

static long long post_check_selection(smcpp_im *im, int c, long long start, long long stop, long long step) {
    const long long L = im->user_Ls[c];
    if (start < 0) throw std::runtime_error("posterior products: start < 0");
    if (stop > L + 1) throw std::runtime_error("posterior products: stop > L + 1 (the contig has " + std::to_string(L + 1) + " columns)");
    if (start >= stop) throw std::runtime_error("posterior products: empty column selection (start >= stop)");
    if (step < 1) throw std::runtime_error("posterior products: step < 1");
    return (stop - start + step - 1) / step;
}

// Where the per-row posteriors of contig c lie: [L + 1][Mp] rows of the caller (row 0 unset) and gamma0 for column 0.
smcpp_im::PostSource smcpp_im::post_source(int c) {
    HIPCHK(hipSetDevice(device));
    PostSource s;
    s.L = user_Ls[c];
    s.rows = split_spans ? merged_gamma(c) : (const double *)(d_gamma_rows.p + (size_t)contig_base[c] * Mp);
    s.g0 = d_gamma0.p + (size_t)c * Mp;
    return s;
}

// gamma or p on a column selection, transposed on the device (k_post_columns) and copied out; the arguments have been checked.
void smcpp_im::post_columns(int c, long long start, long long stop, long long step, bool normalize, bool f32, void *out, double *colsum) {
    const PostSource src = post_source(c);
    PostSel sel;
    sel.start = start; sel.step = step; sel.ncols = (stop - start + step - 1) / step;
    const size_t cells = (size_t)M * sel.ncols;
    if (out) d_post_out.alloc(f32 ? (cells + 1) / 2 : cells);
    if (colsum) d_post_colsum.alloc((size_t)sel.ncols);
    const int need_sum = (normalize && out) || colsum;
    const dim3 grid((unsigned)ceil_div(sel.ncols, PC_TL));
    if (f32)
        hipLaunchKernelGGL(k_post_columns<float>, grid, dim3(256), 0, stream, M, Mp, sel, src.rows, src.g0, need_sum, (int)normalize,
                           out ? (float *)d_post_out.p : (float *)nullptr, colsum ? d_post_colsum.p : (double *)nullptr);
    else
        hipLaunchKernelGGL(k_post_columns<double>, grid, dim3(256), 0, stream, M, Mp, sel, src.rows, src.g0, need_sum, (int)normalize,
                           out ? d_post_out.p : (double *)nullptr, colsum ? d_post_colsum.p : (double *)nullptr);
    HIPCHK(hipGetLastError());
    if (out) HIPCHK(hipMemcpyAsync(out, d_post_out.p, cells * (f32 ? sizeof(float) : sizeof(double)), hipMemcpyDeviceToHost, stream));
    if (colsum) HIPCHK(hipMemcpyAsync(colsum, d_post_colsum.p, sizeof(double) * sel.ncols, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
}

int smcpp_get_gamma(smcpp_im *im, int c, double *out) {
    API_BEGIN
    if (c < 0 || c >= im->n_contigs) throw std::runtime_error("contig index out of range");
    const int M = im->M;
    im->fetch_stats();
    if (!im->gamma_valid) {
        std::memcpy(out, &im->h_gamma0[(size_t)c * M], sizeof(double) * M);   // gamma is M x 1 (hmm.cpp:12-14)
        return 0;
    }
    // every column, as stored: the transpose runs on the device (k_post_columns; rows cut into pieces are added up first)
    im->post_columns(c, 0, (long long)im->user_Ls[c] + 1, 1, false, false, out, nullptr);
    API_END
}

int smcpp_posterior_columns(smcpp_im *im, int c, long long start, long long stop, long long step, int normalize, int f32, void *out,
                            double *colsum) {
    API_BEGIN
    post_need_gamma(im, c);
    post_check_selection(im, c, start, stop, step);
    if (!out && !colsum) return 0;
    im->post_columns(c, start, stop, step, normalize != 0, f32 != 0, out, colsum);
    API_END
}

int smcpp_posterior_summary(smcpp_im *im, int c, long long start, long long stop, long long step, const double *weights, int nq,
                            const double *q, double *colsum, int *argmax, double *mean, int *qstate) {
    API_BEGIN
    post_need_gamma(im, c);
    PostSel sel;
    sel.start = start; sel.step = step; sel.ncols = post_check_selection(im, c, start, stop, step);
    PostLevels lv = check_levels("posterior summary", nq, q);
    const int M = im->M;
    check_weights("posterior summary", weights, M);
    const bool want_mean = weights && mean, want_q = nq > 0 && qstate;
    if (!colsum && !argmax && !want_mean && !want_q) return 0;
    const smcpp_im::PostSource src = im->post_source(c);
    hipStream_t s = im->stream;
    if (colsum) im->d_post_colsum.alloc((size_t)sel.ncols);
    if (argmax) im->d_post_arg.alloc((size_t)sel.ncols);
    if (want_mean) {
        im->d_post_mean.alloc((size_t)sel.ncols);
        im->d_post_w.alloc((size_t)M);
        HIPCHK(hipMemcpyAsync(im->d_post_w.p, weights, sizeof(double) * M, hipMemcpyHostToDevice, s));
    }
    if (want_q) im->d_post_q.alloc((size_t)nq * sel.ncols);
    else lv.nq = 0;
    hipLaunchKernelGGL(k_post_summary, dim3((unsigned)ceil_div(sel.ncols, PS_TL)), dim3(256), 0, s, M, im->Mp, sel, src.rows, src.g0,
                       want_mean ? (const double *)im->d_post_w.p : (const double *)nullptr, lv,
                       colsum ? im->d_post_colsum.p : (double *)nullptr, argmax ? im->d_post_arg.p : (int *)nullptr,
                       want_mean ? im->d_post_mean.p : (double *)nullptr, want_q ? im->d_post_q.p : (int *)nullptr);
    HIPCHK(hipGetLastError());
    if (colsum) HIPCHK(hipMemcpyAsync(colsum, im->d_post_colsum.p, sizeof(double) * sel.ncols, hipMemcpyDeviceToHost, s));
    if (argmax) HIPCHK(hipMemcpyAsync(argmax, im->d_post_arg.p, sizeof(int) * sel.ncols, hipMemcpyDeviceToHost, s));
    if (want_mean) HIPCHK(hipMemcpyAsync(mean, im->d_post_mean.p, sizeof(double) * sel.ncols, hipMemcpyDeviceToHost, s));
    if (want_q) HIPCHK(hipMemcpyAsync(qstate, im->d_post_q.p, sizeof(int) * (size_t)nq * sel.ncols, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

int smcpp_posterior_windows(smcpp_im *im, int c, long long window_bp, long long *n_windows, double *out) {
    API_BEGIN
    post_need_gamma(im, c);
    const long long nwin = window_count(im, c, window_bp, "posterior windows", n_windows);
    if (!out) return 0;
    if (nwin > (1LL << 31) - 1 - PW_WPB) throw std::runtime_error("posterior windows: too many windows for one launch (widen the window)");
    const smcpp_im::PostSource src = im->post_source(c);
    hipStream_t s = im->stream;
    const int M = im->M, Mp = im->Mp;
    const long long L = im->user_Ls[c];
    const long long *P = im->user_prefix_dev(c);
    const double *colsum = im->post_colsum(c, src, im->d_post_colsum);
    im->d_post_out.alloc((size_t)M * nwin);
    hipLaunchKernelGGL(k_post_windows, dim3((unsigned)ceil_div(nwin, PW_WPB), (unsigned)ceil_div(M, 64)), dim3(256), 0, s, M, Mp, L,
                       window_bp, nwin, P, src.rows, colsum, im->d_post_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, im->d_post_out.p, sizeof(double) * (size_t)M * nwin, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

// ---- posterior transition products (posterior_trans_dev.hpp) ----
void smcpp_im::post_transitions_check() {
    if (dirty)
        throw std::runtime_error("posterior transitions: the parameters were set again after the last E-step, whose stored vectors "
                                 "belong to the earlier ones: run the E-step again");
    // the scan chains of the last E-step ran on these generators; an E-step on the dense kernels (long un-cut rows beyond 64
    // states, SMCPP_SS=0, SMCPP_CHAIN, SMCPP_HYBRID=0) stored the same vectors: its T is looked at here
    if (!estep_route.ss_active && !ss_generators_only())
        throw std::runtime_error("posterior transitions: the transition matrix does not have the semiseparable structure of the "
                                 "model's (smcpp_set_raw with an arbitrary matrix): the O(M) steps that walk a row's interior do "
                                 "not exist for it");
    if ((int)ss_gen.size() != 10 * 64 * NPL) throw std::runtime_error("posterior transitions: the generators of T are missing");
}

// stay / up / down of caller's rows start, start + step, .. (ncols of them) of contig c: [3][ncols] on the device, on `stream`.
// The arguments have been checked.
const double *smcpp_im::post_transitions(int c, long long start, long long step, long long ncols) {
    HIPCHK(hipSetDevice(device));
    const int MS = 64 * NPL, Le = Ls[c];
    const int *first = piece_first_dev(c);
    const SsArgs sa = walk_generators();
    PtArgs pa;
    pa.w = walk_rows(c); pa.L = Le;
    pa.nck = walk_checkpoints(longest_row(c), PT_BLK);
    // one wavefront per row, persistent; fewer of them where the scratch of a wavefront is large (many states per lane, or the
    // checkpoints of a very long row): at most 1 GiB in all
    const size_t per_wave = (size_t)PT_BLK * 3 * MS * sizeof(float) + (size_t)pa.nck * MS * sizeof(double);
    const int nw = walk_waves(Le, walk_slots(), per_wave);
    d_pt_park.alloc((size_t)nw * PT_BLK * 3 * MS);
    d_pt_ckpt.alloc(std::max<size_t>(1, (size_t)nw * pa.nck * MS));
    d_pt_eng.alloc((size_t)3 * (Le + 1));
    pa.park = d_pt_park.p; pa.ckpt = d_pt_ckpt.p; pa.out = d_pt_eng.p;
    pt_waves = nw;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    for_npl(NPL, [&](auto x) { hipLaunchKernelGGL((k_post_transitions<decltype(x)::value>), grid, block, 0, stream, sa, pa, nw); });
    HIPCHK(hipGetLastError());
    PostSel sel;
    sel.start = start; sel.step = step; sel.ncols = ncols;
    d_pt_sel.alloc((size_t)3 * ncols);
    hipLaunchKernelGGL(k_post_transitions_select, dim3((unsigned)ceil_div(ncols, 256)), dim3(256), 0, stream, sel, (long long)Le, first,
                       (const double *)d_pt_eng.p, d_pt_sel.p);
    HIPCHK(hipGetLastError());
    return d_pt_sel.p;
}

int smcpp_posterior_transitions(smcpp_im *im, int c, long long start, long long stop, long long step, double *stay, double *up,
                                double *down) {
    API_BEGIN
    post_need_gamma(im, c);
    const long long ncols = post_check_selection(im, c, start, stop, step);
    im->post_transitions_check();
    if (!stay && !up && !down) return 0;
    const double *d = im->post_transitions(c, start, step, ncols);
    hipStream_t s = im->stream;
    double *dst[3] = {stay, up, down};
    for (int x = 0; x < 3; ++x)
        if (dst[x]) HIPCHK(hipMemcpyAsync(dst[x], d + (size_t)x * ncols, sizeof(double) * ncols, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

int smcpp_posterior_transition_windows(smcpp_im *im, int c, long long window_bp, long long *n_windows, double *out) {
    API_BEGIN
    post_need_gamma(im, c);
    const long long nwin = window_count(im, c, window_bp, "posterior transition windows", nullptr);
    im->post_transitions_check();
    if (n_windows) *n_windows = nwin;                  // (a refused call leaves it alone)
    if (!out) return 0;
    if (nwin > 4 * ((1LL << 31) - 1)) throw std::runtime_error("posterior transition windows: too many windows for one launch (widen the window)");
    const long long L = im->user_Ls[c];
    const double *v = im->post_transitions(c, 0, 1, L + 1);
    hipStream_t s = im->stream;
    const long long *P = im->user_prefix_dev(c);
    im->d_post_out.alloc((size_t)3 * nwin);
    hipLaunchKernelGGL(k_post_transition_windows, dim3((unsigned)ceil_div(nwin, 4)), dim3(256), 0, s, L, window_bp, nwin, P, v,
                       im->d_post_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, im->d_post_out.p, sizeof(double) * (size_t)3 * nwin, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

// ---- posterior paths (posterior_paths_dev.hpp) ----
static void post_paths_check(long long path0, long long npaths) {
    if (npaths < 1) throw std::runtime_error("posterior paths: n_paths < 1");
    if (path0 < 0) throw std::runtime_error("posterior paths: first_path < 0");
    if (path0 > (1LL << 31) || npaths > (1LL << 31) || path0 + npaths > (1LL << 31))
        throw std::runtime_error("posterior paths: first_path + n_paths > 2^31 (the path index is one 32-bit word of the counter)");
}
static void post_paths_cap(long long npaths, long long per_path, const char *what) {
    if (npaths > ((1LL << 31) - 1) / std::max<long long>(1, per_path))
        throw std::runtime_error(std::string("posterior paths: ") + what + " (" + std::to_string(npaths) + " paths x " +
                                 std::to_string(per_path) + ") exceed the cap of 2^31 - 1 elements per call: ask for fewer paths "
                                 "or a narrower window");
}

// The arguments have been checked (post_need_gamma, post_transitions_check, post_paths_check, the caps); ncols == 0: no per-row
// product, pos1 <= pos0: no per-position product.
smcpp_im::PostPaths smcpp_im::post_paths(int c, unsigned long long seed, long long path0, long long npaths, long long start,
                                         long long step, long long ncols, long long pos0, long long pos1) {
    HIPCHK(hipSetDevice(device));
    const int MS = 64 * NPL, Le = Ls[c];
    const bool want_rows = ncols > 0, want_pos = pos1 > pos0;
    const int smax = longest_row(c);
    PpArgs pa;
    pa.nck = walk_checkpoints(smax, PP_BLK);
    // paths per wavefront: as few as fill the wavefront slots (a batch shares the forward walk, but its paths run one behind the other)
    const long long slots = walk_slots();
    long long batch = opt().has(smcpp_opt::O_PATH_BATCH) ? opt().ll(smcpp_opt::O_PATH_BATCH, 1) : (npaths + slots - 1) / slots;
    batch = std::max<long long>(1, std::min<long long>(64, batch));
    const long long nbatches = (npaths + batch - 1) / batch;
    // scratch per wavefront: one block of parked vectors + the checkpoints of the longest row; at most 1 GiB in all
    const size_t per_wave = (size_t)PP_BLK * MS * sizeof(float) + (size_t)pa.nck * MS * sizeof(double);
    if (per_wave > (1ull << 30))
        throw std::runtime_error("posterior paths: the checkpoints of a row of " + std::to_string(smax) + " positions exceed the scratch "
                                 "cap of 1 GiB");
    const int nw = walk_waves(nbatches, slots, per_wave);
    const int *first = want_rows ? piece_first_dev(c) : nullptr;
    ensure_T();
    if ((int)T.size() != M * M) throw std::runtime_error("posterior paths: the transition matrix is missing");
    std::vector<double> TT((size_t)(M + 1) * MS, 0.0);
    for (int j = 0; j < M; ++j)
        for (int i = 0; i < M; ++i) TT[(size_t)j * MS + i] = T[(size_t)i * M + j];
    for (int i = 0; i < M; ++i) TT[(size_t)M * MS + i] = 1.0;
    d_pp_TT.upload(TT, stream);
    const SsArgs sa = walk_generators();
    pa.M = M; pa.Mp = Mp; pa.L = Le; pa.base = contig_base[c];
    d_pp_park.alloc((size_t)nw * PP_BLK * MS);
    d_pp_ckpt.alloc(std::max<size_t>(1, (size_t)nw * pa.nck * MS));
    if (want_rows) d_pp_eng.alloc((size_t)3 * npaths * (Le + 1));
    if (want_pos) d_pp_pos.alloc((size_t)npaths * (pos1 - pos0));
    pa.rowinfo = d_rowinfo.p; pa.g_span = d_g_span.p; pa.E = d_E.p; pa.alpha = d_alpha.p; pa.TT = d_pp_TT.p;
    pa.park = d_pp_park.p; pa.ckpt = d_pp_ckpt.p;
    pa.k0 = (unsigned)(seed & 0xffffffffull); pa.k1 = (unsigned)(seed >> 32); pa.contig = (unsigned)c;
    pa.path0 = path0; pa.npaths = npaths; pa.nbatches = nbatches; pa.batch = (int)batch;
    pa.N = user_prefix[c][user_Ls[c]];
    pa.pos0 = want_pos ? pos0 : 0; pa.pos1 = want_pos ? pos1 : 0;
    pa.pos_out = want_pos ? d_pp_pos.p : nullptr;
    pa.rows_out = want_rows ? d_pp_eng.p : nullptr;
    pp_batch = (int)batch; pp_batches = nbatches; pp_waves = nw;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    for_npl(NPL, [&](auto x) { hipLaunchKernelGGL((k_post_paths<decltype(x)::value>), grid, block, 0, stream, sa, pa, nw); });
    HIPCHK(hipGetLastError());
    PostPaths r = {nullptr, want_pos ? d_pp_pos.p : nullptr};
    if (want_rows) {
        PostSel sel;
        sel.start = start; sel.step = step; sel.ncols = ncols;
        d_pp_sel.alloc((size_t)3 * npaths * ncols);
        hipLaunchKernelGGL(k_post_paths_select, dim3((unsigned)ceil_div(npaths * ncols, 256)), dim3(256), 0, stream, sel, (long long)Le,
                           npaths, first, (const int *)d_pp_eng.p, d_pp_sel.p);
        HIPCHK(hipGetLastError());
        r.rows = d_pp_sel.p;
    }
    HIPCHK(hipStreamSynchronize(stream));              // (TT is a local: the copy has to be done before it goes)
    return r;
}

int smcpp_posterior_sample_rows(smcpp_im *im, int c, unsigned long long seed, long long path0, long long npaths, long long start,
                                long long stop, long long step, int *state, int *up, int *down) {
    API_BEGIN
    post_need_gamma(im, c);
    const long long ncols = post_check_selection(im, c, start, stop, step);
    im->post_transitions_check();
    post_paths_check(path0, npaths);
    post_paths_cap(npaths, ncols, "the outputs");
    post_paths_cap(npaths, (long long)im->Ls[c] + 1, "the per-row products over the engine's rows");
    if (!state && !up && !down) return 0;
    const smcpp_im::PostPaths r = im->post_paths(c, seed, path0, npaths, start, step, ncols, 0, 0);
    hipStream_t s = im->stream;
    int *dst[3] = {state, up, down};
    const size_t cells = (size_t)npaths * ncols;
    for (int x = 0; x < 3; ++x)
        if (dst[x]) HIPCHK(hipMemcpyAsync(dst[x], r.rows + (size_t)x * cells, sizeof(int) * cells, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

int smcpp_posterior_sample_positions(smcpp_im *im, int c, unsigned long long seed, long long path0, long long npaths, long long pos0,
                                     long long pos1, int *out) {
    API_BEGIN
    post_need_gamma(im, c);
    im->post_transitions_check();
    post_paths_check(path0, npaths);
    check_position_grid(im, "posterior paths", "window of positions", c, pos0, pos1);
    post_paths_cap(npaths, pos1 - pos0, "the outputs");
    if (!out) return 0;
    const smcpp_im::PostPaths r = im->post_paths(c, seed, path0, npaths, 0, 1, 0, pos0, pos1);
    HIPCHK(hipMemcpyAsync(out, r.pos, sizeof(int) * (size_t)npaths * (pos1 - pos0), hipMemcpyDeviceToHost, im->stream));
    HIPCHK(hipStreamSynchronize(im->stream));
    API_END
}

// ---- simulation (simulate_dev.hpp) ----
int smcpp_simulate(smcpp_im *im, int n_contigs, const long long *lengths, int n_alpha, const int *alpha_keys, int quiet,
                   unsigned long long seed, long long contig0, long long rep0, long long nreps, long long cap,
                   const long long *resume_in, int *x0, long long *n_events, long long *pos, int *state, int *key,
                   long long *resume_out) {
    API_BEGIN
    // ---- the arguments: every refusal before anything is launched ----
    if (n_contigs < 1 || !lengths) throw std::runtime_error("simulate: no contig lengths");
    for (int c = 0; c < n_contigs; ++c)
        if (lengths[c] < 1) throw std::runtime_error("simulate: contig " + std::to_string(c) + " has N < 1 positions");
    if (nreps < 1) throw std::runtime_error("simulate: n_replicates < 1");
    if (cap < 1) throw std::runtime_error("simulate: cap < 1 (events per replicate and call)");
    if (rep0 < 0) throw std::runtime_error("simulate: first_replicate < 0");
    if (rep0 > (1LL << 31) || nreps > (1LL << 31) || rep0 + nreps > (1LL << 31))
        throw std::runtime_error("simulate: first_replicate + n_replicates > 2^31 (the replicate index is one 32-bit word of the counter)");
    if (contig0 < 0 || contig0 + n_contigs > (1LL << 32))
        throw std::runtime_error("simulate: the contig index does not fit one 32-bit word of the counter");
    if (n_alpha < 1 || !alpha_keys) throw std::runtime_error("simulate: the alphabet is empty");
    const int M = im->M, K = im->K, A = n_alpha;
    std::vector<unsigned char> seen(K, 0);
    int qa = -1;
    for (int k = 0; k < A; ++k) {
        const int id = alpha_keys[k];
        if (id < 0 || id >= K)
            throw std::runtime_error("simulate: alphabet entry " + std::to_string(k) + " (key index " + std::to_string(id) +
                                     ") is out of range: the manager holds " + std::to_string(K) + " keys");
        if (seen[id]) throw std::runtime_error("simulate: key index " + std::to_string(id) + " is given twice in the alphabet");
        seen[id] = 1;
        if (id == quiet) qa = k;
    }
    if (qa < 0) throw std::runtime_error("simulate: the quiet key (key index " + std::to_string(quiet) + ") is not in the alphabet");
    const long long units = (long long)n_contigs * nreps;
    if (units > ((1LL << 31) - 1) / cap)
        throw std::runtime_error("simulate: the outputs (" + std::to_string(n_contigs) + " contigs x " + std::to_string(nreps) +
                                 " replicates x " + std::to_string(cap) + " events) exceed the cap of 2^31 - 1 elements per call: ask "
                                 "for fewer replicates or a smaller cap");
    if (resume_in)
        for (long long u = 0; u < units; ++u) {
            const long long e = resume_in[3 * u], p = resume_in[3 * u + 1], i = resume_in[3 * u + 2], N = lengths[u / nreps];
            const bool fresh = i == -1 && e == 0 && p == 0;
            if (!fresh && (e < 0 || e > (1LL << 60) || p < 0 || p > N || i < 0 || i >= M))
                throw std::runtime_error("simulate: resume state " + std::to_string(u) + " is not one a call has returned for this contig");
        }
    // ---- the parameters ----
    if (!im->have_raw && !im->have_model) throw std::runtime_error("simulate: parameters are not set (set_params or set_raw first)");
    if (!im->have_raw) im->prepare_params();
    im->sync_host_E();
    im->ensure_T();
    if ((int)im->pi.size() != M || (int)im->T.size() != M * M || im->E.size() != (size_t)K * M)
        throw std::runtime_error("simulate: parameters are not set (set_params or set_raw first)");
    const int NPL = im->NPL, MS = 64 * NPL;
    // per state: the alphabet's mass, s_i = T(i, i) Ebar(q | i), the weight of staying on a loud key (added up without the quiet
    // entry: no cancellation in 1 - Ebar(q | i))
    std::vector<double> EA((size_t)M * A), vec((size_t)2 * M + MS, 0.0), Tp((size_t)M * MS, 0.0);
    for (int m = 0; m < M; ++m) {
        double mass = 0.0, loud = 0.0;
        for (int k = 0; k < A; ++k) {
            const double v = im->E[(size_t)alpha_keys[k] * M + m];
            if (!(v >= 0.0) || !std::isfinite(v))
                throw std::runtime_error("simulate: the emission probability of alphabet entry " + std::to_string(k) + " in state " +
                                         std::to_string(m) + " is negative or not finite");
            EA[(size_t)m * A + k] = v;
            mass += v;
            if (k != qa) loud += v;
        }
        if (!(mass > 0.0))
            throw std::runtime_error("simulate: state " + std::to_string(m) + " gives the alphabet no mass: no observation can be drawn there");
        const double tii = im->T[(size_t)m * M + m];
        const double s = tii * (EA[(size_t)m * A + qa] / mass);
        vec[m] = s > 0.0 ? std::log(s) : -INFINITY;
        vec[(size_t)M + m] = tii * (loud / mass);
        vec[(size_t)2 * M + m] = im->pi[m];
        std::memcpy(&Tp[(size_t)m * MS], &im->T[(size_t)m * M], sizeof(double) * M);
    }
    if (!x0 && !n_events && !pos && !state && !key && !resume_out) return 0;          // (the checks alone)
    if (!x0 || !n_events || !pos || !state || !key || !resume_out) throw std::runtime_error("simulate: an output array is missing");
    // ---- the launch: one persistent wavefront per (contig, replicate), as many as there are wavefront slots ----
    HIPCHK(hipSetDevice(im->device));
    hipStream_t s = im->stream;
    const std::vector<long long> len(lengths, lengths + n_contigs);
    im->d_sim_T.upload(Tp, s); im->d_sim_EA.upload(EA, s); im->d_sim_vec.upload(vec, s); im->d_sim_len.upload(len, s);
    if (resume_in) {
        im->d_sim_rin.alloc((size_t)3 * units);
        HIPCHK(hipMemcpyAsync(im->d_sim_rin.p, resume_in, sizeof(long long) * 3 * units, hipMemcpyHostToDevice, s));
    }
    const size_t cells = (size_t)units * (size_t)cap;
    im->d_sim_x0.alloc((size_t)units); im->d_sim_nev.alloc((size_t)units); im->d_sim_rout.alloc((size_t)3 * units);
    im->d_sim_pos.alloc(cells); im->d_sim_state.alloc(cells); im->d_sim_key.alloc(cells);
    SimArgs sa;
    sa.M = M; sa.MS = MS; sa.A = A; sa.q = qa;
    sa.T = im->d_sim_T.p; sa.EA = im->d_sim_EA.p; sa.ls = im->d_sim_vec.p; sa.wst = im->d_sim_vec.p + M; sa.pi = im->d_sim_vec.p + 2 * (size_t)M;
    sa.len = im->d_sim_len.p;
    sa.k0 = (unsigned)(seed & 0xffffffffull); sa.k1 = (unsigned)(seed >> 32) ^ 0x53494D55u;
    sa.contig0 = (unsigned)contig0;
    sa.rep0 = rep0; sa.nreps = nreps; sa.units = units; sa.cap = cap;
    sa.resume_in = resume_in ? im->d_sim_rin.p : nullptr;
    sa.x0 = im->d_sim_x0.p; sa.nev = im->d_sim_nev.p; sa.pos = im->d_sim_pos.p; sa.state = im->d_sim_state.p; sa.key = im->d_sim_key.p;
    sa.resume_out = im->d_sim_rout.p;
    const int nw = walk_waves(units, im->walk_slots(), 0);        // (units >= 1: n_contigs and n_replicates were checked above)
    im->sim_waves = nw; im->sim_units = units; im->sim_events = 0;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    for_npl(NPL, [&](auto x) { hipLaunchKernelGGL((k_simulate<decltype(x)::value>), grid, block, 0, s, sa, nw); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(x0, im->d_sim_x0.p, sizeof(int) * units, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_events, im->d_sim_nev.p, sizeof(long long) * units, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(resume_out, im->d_sim_rout.p, sizeof(long long) * 3 * units, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pos, im->d_sim_pos.p, sizeof(long long) * cells, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(state, im->d_sim_state.p, sizeof(int) * cells, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(key, im->d_sim_key.p, sizeof(int) * cells, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));                   // (the staged tables are locals: the copies have to be done before they go)
    for (long long u = 0; u < units; ++u) im->sim_events += n_events[u];
    API_END
}

// ---- posterior positions (posterior_pos_dev.hpp) ----
// Positions 0 .. N of contig c; engine row i covers positions q0 + 1 .. q0 + span.  The item table of a grid: the engine rows that
// hold a grid position, ascending - a caller's row of ONE position (and position 0) as a stored item, every other one to walk.
void smcpp_im::post_positions_grid(int c, long long pos0, long long pos1, long long step) {
    const int Le = Ls[c];
    const std::vector<long long> &P = user_prefix[c];
    pq_items.clear();
    pq_start.clear();
    pq_walked = 0; pq_smax = 1; pq_nseg = 0;
    if (pos0 == 0) pq_items.push_back(PqItem{0, 0, 0, 0, 0});
    long long q0 = 0;
    for (int i = 1; i <= Le; ++i) {
        const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
        const int span = ri.gid >= 0 ? groups[ri.gid].span : 1;
        const long long end = q0 + span, lo = std::max(q0 + 1, pos0);
        if (q0 + 1 >= pos1) break;
        if (end >= pos0) {
            const long long g = pos0 + (lo - pos0 + step - 1) / step * step;       // the first grid position of the row, if any
            if (g <= end && g < pos1) {
                const int l = split_spans ? piece_row[c][i] : i;
                if (P[l] - P[l - 1] == 1) pq_items.push_back(PqItem{end, i, l, 0, 0});
                else {
                    pq_items.push_back(PqItem{end, i, -1, 0, 0});
                    ++pq_walked;
                    pq_smax = std::max(pq_smax, span);
                }
            }
        }
        q0 = end;
    }
}

// The item table of the exact windows: the engine rows of every caller's row that a window boundary cuts, each with the index of its
// first segment (a row that reaches into k + 1 windows has k + 1 segments).
void smcpp_im::post_positions_segments(int c, long long W) {
    const int Le = Ls[c];
    const std::vector<long long> &P = user_prefix[c];
    pq_items.clear();
    pq_start.clear();
    pq_walked = 0; pq_smax = 1; pq_nseg = 0;
    long long q0 = 0;
    for (int i = 1; i <= Le; ++i) {
        const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
        const int span = ri.gid >= 0 ? groups[ri.gid].span : 1;
        const long long end = q0 + span;
        const int l = split_spans ? piece_row[c][i] : i;
        if (P[l - 1] / W != (P[l] - 1) / W) {
            if (pq_nseg > (1LL << 31) - 1 - ((end - 1) / W - q0 / W + 1))
                throw std::runtime_error("posterior positions: more than 2^31 - 1 segments of cut rows (widen the window)");
            pq_items.push_back(PqItem{end, i, -1, (int)pq_nseg, 0});
            pq_start.push_back(q0);
            pq_nseg += (end - 1) / W - q0 / W + 1;
            ++pq_walked;
            pq_smax = std::max(pq_smax, span);
        }
        q0 = end;
    }
}

void smcpp_im::post_positions_scratch_check(size_t extra_bytes) {
    const size_t MS = (size_t)64 * NPL;
    const size_t per_wave = (size_t)PQ_BLK * MS * sizeof(float) + (size_t)walk_checkpoints(pq_smax, PQ_BLK) * MS * sizeof(double);
    if (per_wave > (1ull << 30))
        throw std::runtime_error("posterior positions: the checkpoints of a row of " + std::to_string(pq_smax) + " positions exceed the "
                                 "scratch cap of 1 GiB");
    if (extra_bytes > (1ull << 30))
        throw std::runtime_error("posterior positions: the segment sums of the cut rows (" + std::to_string(pq_nseg) + " vectors) exceed "
                                 "the scratch cap of 1 GiB (widen the window)");
}

// the column sums of every caller's row into dst, by the kernel that serves smcpp_posterior_summary: p is the same number in every product
const double *smcpp_im::post_colsum(int c, const PostSource &src, DevBuf<double> &dst) {
    PostSel all;
    all.start = 0; all.step = 1; all.ncols = (long long)user_Ls[c] + 1;
    dst.alloc((size_t)all.ncols);
    hipLaunchKernelGGL(k_post_summary, dim3((unsigned)ceil_div(all.ncols, PS_TL)), dim3(256), 0, stream, M, Mp, all, src.rows, src.g0,
                       (const double *)nullptr, check_levels("", 0, nullptr), dst.p, (int *)nullptr, (double *)nullptr, (int *)nullptr);
    HIPCHK(hipGetLastError());
    return dst.p;
}

// Launches k_post_positions over pq_items (not empty) with sink `kind`; the sink's fields of pa are the caller's, the rest is set here.
// The arguments have been checked.
void smcpp_im::post_positions_launch(int c, int kind, PqArgs &pa) {
    const int MS = 64 * NPL;
    const SsArgs sa = walk_generators();
    pa.M = M; pa.Mp = Mp; pa.base = contig_base[c];
    pa.nck = walk_checkpoints(pq_smax, PQ_BLK);
    pa.nitems = (int)pq_items.size();
    // one wavefront per item, persistent; fewer of them where the scratch of a wavefront is large: at most 1 GiB in all
    const size_t per_wave = (size_t)PQ_BLK * MS * sizeof(float) + (size_t)pa.nck * MS * sizeof(double);
    const int nw = walk_waves(pa.nitems, walk_slots(), per_wave);
    d_pq_items.upload(pq_items, stream);               // (a member: it outlives the copy)
    d_pq_park.alloc((size_t)nw * PQ_BLK * MS);
    d_pq_ckpt.alloc(std::max<size_t>(1, (size_t)nw * pa.nck * MS));
    pa.rowinfo = d_rowinfo.p; pa.g_span = d_g_span.p; pa.E = d_E.p; pa.alpha = d_alpha.p; pa.beta = d_beta.p;
    pa.items = d_pq_items.p; pa.park = d_pq_park.p; pa.ckpt = d_pq_ckpt.p;
    pq_waves = nw;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    auto launch = [&](auto sink) {
        for_npl(NPL, [&](auto x) {
            hipLaunchKernelGGL((k_post_positions<decltype(x)::value, decltype(sink)>), grid, block, 0, stream, sa, pa, nw);
        });
    };
    if (kind == 0) launch(PqColumns());
    else if (kind == 1) launch(PqSummary());
    else launch(PqSegments());
    HIPCHK(hipGetLastError());
}

static void post_positions_cap(long long per_pos, long long npos, const char *what) {
    if (npos > ((1LL << 31) - 1) / std::max<long long>(1, per_pos))
        throw std::runtime_error(std::string("posterior positions: ") + what + " (" + std::to_string(per_pos) + " x " +
                                 std::to_string(npos) + " positions) exceed the cap of 2^31 - 1 elements per array: ask for a "
                                 "narrower or a coarser grid");
}

int smcpp_posterior_positions(smcpp_im *im, int c, long long pos0, long long pos1, long long step, double *out) {
    API_BEGIN
    post_need_gamma(im, c);
    im->post_transitions_check();
    const long long npos = check_position_grid(im, "posterior positions", "grid", c, pos0, pos1, step);
    post_positions_cap(im->M, npos, "the columns");
    im->post_positions_grid(c, pos0, pos1, step);
    im->post_positions_scratch_check(0);
    if (!out) return 0;
    const smcpp_im::PostSource src = im->post_source(c);
    PqArgs pa = PqArgs();
    pa.rows = src.rows; pa.g0 = src.g0; pa.colsum = im->post_colsum(c, src, im->d_pq_colsum);
    pa.pos0 = pos0; pa.pos1 = pos1; pa.step = step; pa.npos = npos;
    const size_t cells = (size_t)im->M * npos;
    im->d_post_out.alloc(cells);
    pa.out = im->d_post_out.p;
    im->post_positions_launch(c, 0, pa);
    HIPCHK(hipMemcpyAsync(out, im->d_post_out.p, sizeof(double) * cells, hipMemcpyDeviceToHost, im->stream));
    HIPCHK(hipStreamSynchronize(im->stream));
    API_END
}

int smcpp_posterior_position_summary(smcpp_im *im, int c, long long pos0, long long pos1, long long step, const double *weights, int nq,
                                     const double *q, int *argmax, double *mean, int *qstate) {
    API_BEGIN
    post_need_gamma(im, c);
    im->post_transitions_check();
    const long long npos = check_position_grid(im, "posterior positions", "grid", c, pos0, pos1, step);
    PqArgs pa = PqArgs();
    pa.lv = check_levels("posterior position summary", nq, q);
    const int M = im->M;
    check_weights("posterior position summary", weights, M);
    post_positions_cap(std::max(1, nq), npos, "the summaries");
    im->post_positions_grid(c, pos0, pos1, step);
    im->post_positions_scratch_check(0);
    const bool want_mean = weights && mean, want_q = nq > 0 && qstate;
    if (!argmax && !want_mean && !want_q) return 0;
    const smcpp_im::PostSource src = im->post_source(c);
    hipStream_t s = im->stream;
    pa.rows = src.rows; pa.g0 = src.g0; pa.colsum = im->post_colsum(c, src, im->d_pq_colsum);
    pa.pos0 = pos0; pa.pos1 = pos1; pa.step = step; pa.npos = npos;
    if (argmax) { im->d_post_arg.alloc((size_t)npos); pa.argmax = im->d_post_arg.p; }
    if (want_mean) {
        im->d_post_mean.alloc((size_t)npos);
        im->d_post_w.alloc((size_t)M);
        HIPCHK(hipMemcpyAsync(im->d_post_w.p, weights, sizeof(double) * M, hipMemcpyHostToDevice, s));
        pa.w = im->d_post_w.p; pa.mean = im->d_post_mean.p;
    }
    if (want_q) { im->d_post_q.alloc((size_t)nq * npos); pa.qstate = im->d_post_q.p; }
    else pa.lv.nq = 0;
    im->post_positions_launch(c, 1, pa);
    if (argmax) HIPCHK(hipMemcpyAsync(argmax, im->d_post_arg.p, sizeof(int) * npos, hipMemcpyDeviceToHost, s));
    if (want_mean) HIPCHK(hipMemcpyAsync(mean, im->d_post_mean.p, sizeof(double) * npos, hipMemcpyDeviceToHost, s));
    if (want_q) HIPCHK(hipMemcpyAsync(qstate, im->d_post_q.p, sizeof(int) * (size_t)nq * npos, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

int smcpp_posterior_windows_exact(smcpp_im *im, int c, long long window_bp, long long *n_windows, double *out) {
    API_BEGIN
    post_need_gamma(im, c);
    const long long nwin = window_count(im, c, window_bp, "posterior windows", nullptr);
    im->post_transitions_check();
    if (n_windows) *n_windows = nwin;                  // (a refused call leaves it alone)
    if (!out) return 0;
    post_positions_cap(im->M, nwin, "the windows");
    im->post_positions_segments(c, window_bp);
    const int M = im->M, Mp = im->Mp, MS = 64 * im->NPL;
    im->post_positions_scratch_check((size_t)im->pq_nseg * MS * sizeof(double));
    const smcpp_im::PostSource src = im->post_source(c);
    hipStream_t s = im->stream;
    const long long L = im->user_Ls[c];
    const long long *P = im->user_prefix_dev(c);
    const double *colsum = im->post_colsum(c, src, im->d_pq_colsum);
    const int nit = (int)im->pq_items.size();
    im->d_pq_seg.alloc(std::max<size_t>(1, (size_t)im->pq_nseg * MS));
    im->d_pq_start.upload(im->pq_start, s);            // (a member: it outlives the copy)
    if (nit > 0) {
        PqArgs pa = PqArgs();
        pa.W = window_bp; pa.seg = im->d_pq_seg.p;
        pa.step = 1;
        im->post_positions_launch(c, 2, pa);
    } else {
        im->pq_waves = 0;
        im->d_pq_items.alloc(1);
        im->d_pq_start.alloc(1);
    }
    im->d_post_out.alloc((size_t)M * nwin);
    hipLaunchKernelGGL(k_post_windows_exact, dim3((unsigned)ceil_div(nwin, 4), (unsigned)ceil_div(M, 64)), dim3(256), 0, s, M, Mp, MS, L,
                       window_bp, nwin, P, src.rows, colsum, (const PqItem *)im->d_pq_items.p,
                       (const long long *)im->d_pq_start.p, nit, (const double *)im->d_pq_seg.p, im->d_post_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, im->d_post_out.p, sizeof(double) * (size_t)M * nwin, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

// ---- log-likelihood track (loglik_track_dev.hpp) ----
// Every E-step plan leaves the float alpha and log c of every engine row in memory (the statistics read both), so a plain E-step
// is enough; `walk`: the call steps through the interior of rows and needs the generators of a structured T as well.
static void ll_need_estep(smcpp_im *im, int c, bool walk) {
    if (!im->estep_done) throw std::runtime_error("loglik track: no E-step has been run on this manager yet");
    if (c < 0 || c >= im->n_contigs) throw std::runtime_error("contig index out of range");
    if (walk) im->post_transitions_check();
    else if (im->dirty)
        throw std::runtime_error("loglik track: the parameters were set again after the last E-step, whose stored values belong to the "
                                 "earlier ones: run the E-step again");
}

// The position prefix of the engine's rows of contig c: the caller's where no row is cut.
const long long *smcpp_im::ll_epos_dev(int c) {
    if (!split_spans) return user_prefix_dev(c);
    if (d_ll_epos.size() != (size_t)n_contigs) d_ll_epos.resize(n_contigs);
    if (!d_ll_epos[c].p) {
        const int Le = Ls[c];
        std::vector<long long> ep((size_t)Le + 1, 0);
        for (int i = 1; i <= Le; ++i) {
            const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
            ep[i] = ep[i - 1] + (ri.gid >= 0 ? groups[ri.gid].span : 1);
        }
        d_ll_epos[c].upload(ep, stream);
        HIPCHK(hipStreamSynchronize(stream));          // (`ep` is a local: the copy has to be done before it goes)
    }
    return d_ll_epos[c].p;
}

// pre[i] = sum of log c over the engine rows 1 .. i of contig c, pre[0] = 0: block sums, one block over them, downsweep
const double *smcpp_im::ll_prefix(int c) {
    HIPCHK(hipSetDevice(device));
    const long long Le = Ls[c];
    const int nb = std::max(1, ceil_div(Le, LL_SCAN_BLOCK));
    const double *v = d_logc.p + (size_t)contig_base[c];
    d_ll_part.alloc((size_t)nb);
    d_ll_pre.alloc((size_t)Le + 1);
    hipLaunchKernelGGL(k_ll_scan_partials, dim3(nb), dim3(LL_SCAN_BLOCK), 0, stream, Le, v, d_ll_part.p);
    hipLaunchKernelGGL(k_ll_scan_of_partials, dim3(1), dim3(LL_SCAN_BLOCK), 0, stream, (long long)nb, d_ll_part.p);
    hipLaunchKernelGGL(k_ll_scan_down, dim3(nb), dim3(LL_SCAN_BLOCK), 0, stream, Le, v, (const double *)d_ll_part.p, d_ll_pre.p);
    HIPCHK(hipGetLastError());
    return d_ll_pre.p;
}

// The item table: the engine rows with a query position STRICTLY inside, ascending.  Grid: the queries are pos0, pos0 + step, ..
// < pos1 and query j owns slot j; windows: the queries are the boundaries step, 2 step, .. < N and the slots are counted.
// The builder is shared with the score track's exact windows, which keep a table of their own (`items`, `nslots`: the caller's).
void smcpp_im::walk_item_table(int c, long long pos0, long long pos1, long long step, bool windows, std::vector<LlItem> &items,
                               long long &nslots) const {
    const int Le = Ls[c];
    items.clear();
    nslots = 0;
    long long q0 = 0;
    for (int i = 1; i <= Le; ++i) {
        const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
        const int span = ri.gid >= 0 ? groups[ri.gid].span : 1;
        const long long end = q0 + span;
        if (q0 + 1 >= pos1) break;
        if (span > 1 && end - 1 >= pos0) {
            const long long lo = std::max(q0 + 1, pos0);
            const long long g = pos0 + (lo - pos0 + step - 1) / step * step;      // the first query behind q0, if any
            if (g < end && g < pos1) {
                const long long last = std::min(end - 1, pos1 - 1);
                const int nq = (int)((last - g) / step + 1);
                items.push_back(LlItem{q0, g, windows ? nslots : (g - pos0) / step, i, nq});
                nslots += nq;
            }
        }
        q0 = end;
    }
}
void smcpp_im::ll_table(int c, long long pos0, long long pos1, long long step, bool windows) {
    walk_item_table(c, pos0, pos1, step, windows, ll_items, ll_nslots);
}

void smcpp_im::ll_walk(int c, long long step, double *slots) {
    const SsArgs sa = walk_generators();
    LlArgs la = LlArgs();
    la.w = walk_rows(c); la.w.beta = nullptr;          // (forward only: whether the last E-step kept beta does not matter)
    la.nitems = (int)ll_items.size(); la.logc = d_logc.p; la.pre = d_ll_pre.p;
    d_ll_items.upload(ll_items, stream);               // (a member: it outlives the copy)
    d_ll_ratio.alloc((size_t)la.nitems);
    la.items = d_ll_items.p; la.step = step; la.out = slots; la.ratio = d_ll_ratio.p;
    // one wavefront per item, persistent: as many as there are wavefront slots, or as SMCPP_LL_WAVES allows
    long long nw = walk_waves(la.nitems, walk_slots(), 0);
    if (opt().has(smcpp_opt::O_LL_WAVES)) nw = std::min(nw, std::max<long long>(1, opt().ll(smcpp_opt::O_LL_WAVES, 1)));
    ll_waves = (int)nw;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    for_npl(NPL, [&](auto x) { hipLaunchKernelGGL((k_ll_walk<decltype(x)::value>), grid, block, 0, stream, sa, la, (int)nw); });
    HIPCHK(hipGetLastError());
    ll_ratio_h.resize((size_t)la.nitems);
    HIPCHK(hipMemcpyAsync(ll_ratio_h.data(), d_ll_ratio.p, sizeof(double) * la.nitems, hipMemcpyDeviceToHost, stream));
}

// (behind the stream's synchronisation) the worst ratio of the walk that has just run
static void ll_close(smcpp_im *im, bool walked) {
    im->ll_nitems = walked ? (long long)im->ll_items.size() : 0;
    if (!walked) im->ll_waves = 0;
    double w = 0.0;
    if (walked)
        for (double r : im->ll_ratio_h) w = (r > w || r != r) ? r : w;
    im->ll_worst = std::isfinite(w) ? w : 1e300;
}

static void ll_cap(long long n, const char *what) {
    if (n > (1LL << 31) - 1)
        throw std::runtime_error(std::string("loglik track: ") + what + " (" + std::to_string(n) + ") exceed the cap of 2^31 - 1 elements "
                                 "per call: ask for a narrower or a coarser grid, or a wider window");
}

int smcpp_loglik_rows(smcpp_im *im, int c, long long start, long long stop, long long step, double *out) {
    API_BEGIN
    ll_need_estep(im, c, false);
    const long long ncols = post_check_selection(im, c, start, stop, step);
    if (!out) return 0;
    const double *pre = im->ll_prefix(c);              // (selects the device)
    const int *first = im->piece_first_dev(c);
    im->d_ll_out.alloc((size_t)ncols);
    hipLaunchKernelGGL(k_ll_rows, dim3((unsigned)ceil_div(ncols, 256)), dim3(256), 0, im->stream, start, step, ncols, first, pre,
                       im->d_ll_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, im->d_ll_out.p, sizeof(double) * (size_t)ncols, hipMemcpyDeviceToHost, im->stream));
    HIPCHK(hipStreamSynchronize(im->stream));
    ll_close(im, false);
    API_END
}

int smcpp_loglik_positions(smcpp_im *im, int c, long long pos0, long long pos1, long long step, double *out) {
    API_BEGIN
    ll_need_estep(im, c, true);
    const long long npos = check_position_grid(im, "loglik track", "grid", c, pos0, pos1, step);
    ll_cap(npos, "the grid positions");
    if (!out) return 0;
    im->ll_table(c, pos0, pos1, step, false);
    const double *pre = im->ll_prefix(c);              // (selects the device)
    const long long *EP = im->ll_epos_dev(c);
    hipStream_t s = im->stream;
    im->d_ll_out.alloc((size_t)npos);
    hipLaunchKernelGGL(k_ll_ends, dim3((unsigned)ceil_div(npos, 256)), dim3(256), 0, s, pos0, step, npos, (long long)im->Ls[c], EP, pre,
                       im->d_ll_out.p);
    HIPCHK(hipGetLastError());
    const bool walked = !im->ll_items.empty();
    if (walked) im->ll_walk(c, step, im->d_ll_out.p);
    HIPCHK(hipMemcpyAsync(out, im->d_ll_out.p, sizeof(double) * (size_t)npos, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ll_close(im, walked);
    API_END
}

int smcpp_loglik_windows(smcpp_im *im, int c, long long window_bp, long long *n_windows, double *out) {
    API_BEGIN
    ll_need_estep(im, c, true);
    const long long nwin = window_count(im, c, window_bp, "loglik track", n_windows);
    const long long N = im->user_prefix[c][im->user_Ls[c]];
    ll_cap(nwin, "the windows");
    if (!out) return 0;
    im->ll_table(c, 0, N, window_bp, true);            // (the boundaries W, 2 W, .. < N)
    const double *pre = im->ll_prefix(c);              // (selects the device)
    const long long *EP = im->ll_epos_dev(c);
    hipStream_t s = im->stream;
    const bool walked = !im->ll_items.empty();
    im->d_ll_bnd.alloc(std::max<size_t>(1, (size_t)im->ll_nslots));
    if (walked) im->ll_walk(c, window_bp, im->d_ll_bnd.p);
    else im->d_ll_items.alloc(1);
    im->d_ll_out.alloc(std::max<size_t>(1, (size_t)nwin));
    if (nwin > 0) {
        hipLaunchKernelGGL(k_ll_windows, dim3((unsigned)ceil_div(nwin, 256)), dim3(256), 0, s, window_bp, nwin, (long long)im->Ls[c], EP, pre,
                           (const LlItem *)im->d_ll_items.p, (int)im->ll_items.size(), (const double *)im->d_ll_bnd.p, im->d_ll_out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, im->d_ll_out.p, sizeof(double) * (size_t)nwin, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    ll_close(im, walked);
    API_END
}

// ---- score track (score_track_dev.hpp) ----
// Everything a score call needs besides its own arguments; -> the checkpoint vectors a wavefront needs on contig c.
int smcpp_im::score_check(int c) {
    if (!estep_done) throw std::runtime_error("score track: no E-step has been run on this manager yet");
    if (!gamma_valid) throw std::runtime_error("score track: save_gamma was not set for the last E-step");
    if (c < 0 || c >= n_contigs) throw std::runtime_error("contig index out of range");
    if (dirty)
        throw std::runtime_error("score track: the parameters were set again after the last E-step, whose stored vectors belong to the "
                                 "earlier ones: run the E-step again");
    // the walk is the transition products': the same structure of T (what an arbitrary smcpp_set_raw matrix lacks), the same generators
    try { post_transitions_check(); }
    catch (const std::runtime_error &e) { throw std::runtime_error(std::string("score track: ") + e.what()); }
    if (have_raw)
        throw std::runtime_error("score track: the parameters were set with smcpp_set_raw: no model, no derivative seeds");
    if (nder < 1)
        throw std::runtime_error("score track: the parameters carry no derivative seeds (nder = 0): set them with seeds and run the "
                                 "E-step again");
    const bool vec = score_form_vectors();
    // (the matrix form's refusal keeps its text to the letter - tests/test_gpu_product_refusals.py holds it; SMCPP_SCORE_FORM=vectors,
    // the way past 64 states, is named in the header, the README and the switch table)
    if (!vec && (M > 64 || NPL != 1))
        throw std::runtime_error("score track: more than 64 hidden states (" + std::to_string(M) + "): the kernel keeps one column of the "
                                 "M x M accumulator per lane and exists at one state per lane only");
    if (vec) {
        const std::string who = "score track (SMCPP_SCORE_FORM=vectors): ";
        if (NPL > 4)
            throw std::runtime_error(who + "more than 256 hidden states (" + std::to_string(M) + "): the kernel exists at one to four "
                                     "states per lane; use fewer hidden states");
        HIPCHK(hipSetDevice(device));
        prepare_params();                              // (fresh since the E-step: !dirty)
        if (!tgen_valid || !tgen.ok || tgen.M != M || tgen.nder != nder)
            throw std::runtime_error(who + "the generator planes of the transition Jacobian do not exist for the last E-step's parameters "
                                     "(a model prepared on the host - SMCPP_PREP=host -, a two-population manager, or a transition matrix "
                                     "that needed the pairwise fallback): " +
                                     (M <= 64 ? "unset SMCPP_SCORE_FORM, the matrix form serves this manager"
                                              : "prepare a one-population model on the device (unset SMCPP_PREP) and run the E-step again"));
    }
    const int smax = longest_row(c), nck = walk_checkpoints(smax, SC_BLK);
    // scratch: the three parts of every direction per engine row + one wavefront's checkpoints (and parked block) at the least
    const size_t MS = (size_t)64 * NPL;
    const size_t bytes = ((size_t)3 * nder * ((size_t)Ls[c] + 1) + (size_t)nck * MS) * sizeof(double) +
                         (vec ? (size_t)SV_BLK * 4 * MS * sizeof(float) : 0);
    if (bytes > (1ull << 30))
        throw std::runtime_error("score track: the scratch (" + std::to_string(nder) + " directions x 3 parts x " + std::to_string(Ls[c] + 1) +
                                 " engine rows, the checkpoints of a row of " + std::to_string(smax) + " positions) exceeds the cap of 1 GiB");
    return nck;
}

static void score_cap(long long per_col, long long ncols, const char *what) {
    if (ncols > ((1LL << 31) - 1) / std::max<long long>(1, per_col))
        throw std::runtime_error(std::string("score track: ") + what + " (" + std::to_string(per_col) + " x " + std::to_string(ncols) +
                                 ") exceed the cap of 2^31 - 1 elements per call: ask for a narrower selection or a wider window");
}

bool smcpp_im::score_form_vectors() const {
    if (!opt().has(smcpp_opt::O_SCORE_FORM) || opt().is(smcpp_opt::O_SCORE_FORM, "matrix")) return false;
    if (opt().is(smcpp_opt::O_SCORE_FORM, "vectors")) return true;
    throw std::runtime_error("score track: SMCPP_SCORE_FORM is 'matrix' or 'vectors', not '" + opt().str(smcpp_opt::O_SCORE_FORM) + "'");
}

// G_pi [nder][64] | dT [nder][64][64] | G_E [K][nder][64] from the host arrays the Jacobian getters copy out, zero beyond M and
// where a value is not positive.  A device-prepared emission table is FETCHED into locals: E_on_dev stays as it is.
void smcpp_im::score_tables() {
    if (sc_tab_valid) return;
    HIPCHK(hipSetDevice(device));
    prepare_params();                                  // (fresh since the E-step: !dirty)
    ensure_dT();
    std::vector<double> Eloc, dEloc;
    const std::vector<double> *Ev = &E, *dEv = &dE;
    if (E_on_dev) {
        fetch_prepared_table(Eloc, dEloc, false);          // (the table and its Jacobian alone; nder >= 1 here: score_check)
        Ev = &Eloc; dEv = &dEloc;
    }
    const size_t nd = (size_t)nder;
    if (dpi.size() != (size_t)M * nd || dT.size() != (size_t)M * M * nd || Ev->size() != (size_t)K * M || dEv->size() != (size_t)K * M * nd)
        throw std::runtime_error("score track: the Jacobians of pi, T and E are not available for the last E-step's parameters");
    std::vector<double> tab(nd * 64 + nd * 64 * 64 + (size_t)K * nd * 64, 0.0);
    double *gp = tab.data(), *gt = gp + nd * 64, *ge = gt + nd * 64 * 64;
    for (int d = 0; d < nder; ++d) {
        for (int i = 0; i < M; ++i) gp[d * 64 + i] = pi[i] > 0.0 ? dpi[(size_t)i * nd + d] / pi[i] : 0.0;
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < M; ++j) gt[((size_t)d * 64 + i) * 64 + j] = dT[((size_t)i * M + j) * nd + d];
        for (int k = 0; k < K; ++k)
            for (int i = 0; i < M; ++i) {
                const double e = (*Ev)[(size_t)k * M + i];
                ge[((size_t)k * nd + d) * 64 + i] = e > 0.0 ? (*dEv)[((size_t)k * M + i) * nd + d] / e : 0.0;
            }
    }
    d_sc_tab.upload(tab, stream);
    HIPCHK(hipStreamSynchronize(stream));              // (`tab` is a local: the copy has to be done before it goes)
    sc_tab_valid = true;
}

// The vector form's tables, MS = 64 NPL wide: G_pi [nder][MS] | cD, cL, cW, cP / d [nder][4][MS] | G_E [K][nder][MS], the last two by
// BACKWARD position (state j at MS - 1 - j, as ss_pack_generators mirrors the backward generators), zero beyond M and where a value
// is not positive.  The transition planes come from the generator planes (score_planes): the dense dT is not expanded.  d is the
// diagonal the walk's generators hold, so that the parked stay addend d_i x(i) times cP(i) / d_i is x(i) cP(i).
void smcpp_im::score_tables_vec() {
    if (sv_tab_valid) return;
    HIPCHK(hipSetDevice(device));
    std::vector<double> Eloc, dEloc;
    const std::vector<double> *Ev = &E, *dEv = &dE;
    if (E_on_dev) {
        fetch_prepared_table(Eloc, dEloc, false);
        Ev = &Eloc; dEv = &dEloc;
    }
    const size_t nd = (size_t)nder, MS = (size_t)64 * NPL;
    if (dpi.size() != (size_t)M * nd || Ev->size() != (size_t)K * M || dEv->size() != (size_t)K * M * nd)
        throw std::runtime_error("score track: the Jacobians of pi and E are not available for the last E-step's parameters");
    const double *diag = &ss_gen[5 * MS];              // f_d (post_transitions_check has seen the generators)
    std::vector<double> pl[4];
    score_planes(tgen, diag, pl[0], pl[1], pl[2], pl[3]);
    std::vector<double> tab(nd * MS + nd * 4 * MS + (size_t)K * nd * MS, 0.0);
    double *gp = tab.data(), *gt = gp + nd * MS, *ge = gt + nd * 4 * MS;
    for (int d = 0; d < nder; ++d)
        for (int i = 0; i < M; ++i) {
            const size_t p = MS - 1 - i;
            gp[d * MS + i] = pi[i] > 0.0 ? dpi[(size_t)i * nd + d] / pi[i] : 0.0;
            for (int q = 0; q < 4; ++q) gt[((size_t)d * 4 + q) * MS + p] = pl[q][(size_t)d * M + i] / (q == 3 ? diag[i] : 1.0);
            for (int k = 0; k < K; ++k) {
                const double e = (*Ev)[(size_t)k * M + i];
                ge[((size_t)k * nd + d) * MS + p] = e > 0.0 ? (*dEv)[((size_t)k * M + i) * nd + d] / e : 0.0;
            }
        }
    d_sv_tab.upload(tab, stream);
    HIPCHK(hipStreamSynchronize(stream));              // (`tab` is a local: the copy has to be done before it goes)
    sv_tab_valid = true;
}

// k_score_rows_vec over the engine rows of contig c -> d_sc_eng.  Scratch as post_transitions sizes it: one persistent wavefront per
// engine row up to walk_slots(), fewer where the parked blocks and checkpoints would pass 1 GiB with the parts, or SMCPP_SCORE_WAVES says so.
void smcpp_im::score_rows_vec(int c, int nck) {
    score_tables_vec();
    const int Le = Ls[c];
    const size_t nd = (size_t)nder, MS = (size_t)64 * NPL;
    const SsArgs sa = walk_generators();
    SvArgs a = SvArgs();
    a.M = M; a.Mp = Mp; a.L = Le; a.nck = nck; a.nder = nder; a.base = contig_base[c];
    const size_t left = (1ull << 30) - (size_t)3 * nd * ((size_t)Le + 1) * sizeof(double);         // (score_check: one wavefront fits)
    const size_t per_wave = (size_t)SV_BLK * 4 * MS * sizeof(float) + (size_t)nck * MS * sizeof(double);
    long long nw = walk_waves(Le, walk_slots(), per_wave, left);
    if (opt().has(smcpp_opt::O_SCORE_WAVES)) nw = std::min(nw, std::max<long long>(1, opt().ll(smcpp_opt::O_SCORE_WAVES, 1)));
    d_sv_park.alloc((size_t)nw * SV_BLK * 4 * MS);
    d_sc_ckpt.alloc(std::max<size_t>(1, (size_t)nw * nck * MS));
    a.rowinfo = d_rowinfo.p; a.g_span = d_g_span.p; a.E = d_E.p; a.alpha = d_alpha.p; a.beta = d_beta.p;
    a.gamma0 = d_gamma0.p + (size_t)c * Mp;
    a.Gpi = d_sv_tab.p; a.planes = a.Gpi + nd * MS; a.GE = a.planes + nd * 4 * MS;
    a.park = d_sv_park.p; a.ckpt = d_sc_ckpt.p; a.out = d_sc_eng.p;
    sc_waves = (int)nw; sc_items = Le;
    const dim3 grid((unsigned)ceil_div(nw, 4)), block(256);
    for_npl(NPL, [&](auto x) {
        constexpr int npl = decltype(x)::value;
        if constexpr (npl <= 4) hipLaunchKernelGGL((k_score_rows_vec<npl>), grid, block, 0, stream, sa, a, (int)nw);   // (score_check: NPL <= 4)
    });
    HIPCHK(hipGetLastError());
}

// The parts (parts != 0: [3][nder][ncols]) or the total ([nder][ncols]) of caller's rows start, start + step, .. of contig c, on the
// device, on `stream`, in the form SMCPP_SCORE_FORM names at this call.  The arguments have been checked (score_check -> nck, the caps).
const double *smcpp_im::score_rows(int c, long long start, long long step, long long ncols, int parts, int nck) {
    HIPCHK(hipSetDevice(device));
    const int Le = Ls[c];
    const int *first = piece_first_dev(c);
    d_sc_eng.alloc((size_t)3 * nder * ((size_t)Le + 1));
    sc_vectors = score_form_vectors();
    if (sc_vectors) score_rows_vec(c, nck);
    else score_rows_matrix(c, nck);
    PostSel sel;
    sel.start = start; sel.step = step; sel.ncols = ncols;
    d_sc_sel.alloc((size_t)(parts ? 3 : 1) * nder * ncols);
    hipLaunchKernelGGL(k_score_select, dim3((unsigned)ceil_div(ncols * nder, 256)), dim3(256), 0, stream, sel, (long long)Le, nder, parts,
                       first, (const double *)d_sc_eng.p, d_sc_sel.p);
    HIPCHK(hipGetLastError());
    return d_sc_sel.p;
}

// k_score_rows (the matrix form, one state per lane: score_check) over the engine rows of contig c -> d_sc_eng.
void smcpp_im::score_rows_matrix(int c, int nck) {
    score_tables();
    const int Le = Ls[c];
    const SsArgs sa = walk_generators();               // (one state per lane: score_check)
    ScArgs a = ScArgs();
    a.w = walk_rows(c); a.L = Le; a.nck = nck; a.nder = nder;
    // one wavefront per engine row, persistent: a workgroup's parked vectors fill a CU's LDS, so 4 wavefronts per CU are resident;
    // fewer where SMCPP_SCORE_WAVES says so or the checkpoints of a very long row would pass 1 GiB with the parts
    const size_t left = (1ull << 30) - (size_t)3 * nder * ((size_t)Le + 1) * sizeof(double);       // (not negative: score_check)
    long long nw = walk_waves(Le, 1024, (size_t)nck * 64 * sizeof(double), left);   // (a contig without rows: wavefront 0 writes column 0)
    if (opt().has(smcpp_opt::O_SCORE_WAVES)) nw = std::min(nw, std::max<long long>(1, opt().ll(smcpp_opt::O_SCORE_WAVES, 1)));
    d_sc_ckpt.alloc(std::max<size_t>(1, (size_t)nw * nck * 64));
    a.gamma0 = d_gamma0.p + (size_t)c * Mp;
    a.Gpi = d_sc_tab.p; a.dT = a.Gpi + (size_t)nder * 64; a.GE = a.dT + (size_t)nder * 64 * 64;
    a.ckpt = d_sc_ckpt.p; a.out = d_sc_eng.p;
    sc_waves = (int)nw; sc_items = Le;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_score_rows), hipFuncAttributeMaxDynamicSharedMemorySize, SC_LDS_BYTES));
    hipLaunchKernelGGL(k_score_rows, dim3((unsigned)ceil_div(nw, 4)), dim3(256), SC_LDS_BYTES, stream, sa, a, (int)nw);
    HIPCHK(hipGetLastError());
}

int smcpp_score_rows(smcpp_im *im, int c, long long start, long long stop, long long step, int parts, double *out) {
    API_BEGIN
    const int nck = im->score_check(c);
    const long long ncols = post_check_selection(im, c, start, stop, step);
    score_cap((parts ? 3LL : 1LL) * im->nder, ncols, "the outputs");
    if (!out) return 0;
    const double *d = im->score_rows(c, start, step, ncols, parts, nck);
    HIPCHK(hipMemcpyAsync(out, d, sizeof(double) * (size_t)(parts ? 3 : 1) * im->nder * ncols, hipMemcpyDeviceToHost, im->stream));
    HIPCHK(hipStreamSynchronize(im->stream));
    API_END
}

int smcpp_score_windows(smcpp_im *im, int c, long long window_bp, long long *n_windows, double *out) {
    API_BEGIN
    const int nck = im->score_check(c);
    const long long nwin = window_count(im, c, window_bp, "score track", n_windows);
    score_cap(im->nder, nwin, "the windows");
    if (!out) return 0;
    const long long L = im->user_Ls[c];
    const double *v = im->score_rows(c, 0, 1, L + 1, 0, nck);
    hipStream_t s = im->stream;
    const long long *P = im->user_prefix_dev(c);
    if (nwin > 0) {                                    // (a contig without rows has no base pairs and no windows)
        im->d_sc_out.alloc((size_t)im->nder * nwin);
        hipLaunchKernelGGL(k_score_windows, dim3((unsigned)ceil_div(nwin, 4)), dim3(256), 0, s, L, window_bp, nwin, im->nder, P, v,
                           im->d_sc_out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, im->d_sc_out.p, sizeof(double) * (size_t)im->nder * nwin, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

// k_score_segments_vec over sx_items -> d_sx_seg [3][nder][sx_nslots], on `stream`, behind the row walk of the same call (whose
// tables, parked blocks and checkpoints it takes over: one stream, one kernel after the other).  nw: the wavefronts, sized by the caller.
void smcpp_im::score_segments_vec(int c, int nck, long long W, long long nw) {
    const size_t nd = (size_t)nder, MS = (size_t)64 * NPL;
    const SsArgs sa = walk_generators();
    SgArgs g = SgArgs();
    SvArgs &a = g.v;
    a.M = M; a.Mp = Mp; a.L = Ls[c]; a.nck = nck; a.nder = nder; a.base = contig_base[c];
    d_sv_park.alloc((size_t)nw * SV_BLK * 4 * MS);
    d_sc_ckpt.alloc(std::max<size_t>(1, (size_t)nw * nck * MS));
    d_sx_items.upload(sx_items, stream);               // (a member: it outlives the copy)
    d_sx_seg.alloc((size_t)3 * nd * (size_t)sx_nslots);
    a.rowinfo = d_rowinfo.p; a.g_span = d_g_span.p; a.E = d_E.p; a.alpha = d_alpha.p; a.beta = d_beta.p;
    a.gamma0 = d_gamma0.p + (size_t)c * Mp;
    a.Gpi = d_sv_tab.p; a.planes = a.Gpi + nd * MS; a.GE = a.planes + nd * 4 * MS;
    a.park = d_sv_park.p; a.ckpt = d_sc_ckpt.p; a.out = nullptr;
    g.nitems = (int)sx_items.size(); g.items = d_sx_items.p; g.W = W; g.nslots = sx_nslots; g.seg = d_sx_seg.p;
    const dim3 grid((unsigned)ceil_div(nw, 4)), block(256);
    for_npl(NPL, [&](auto x) {
        constexpr int npl = decltype(x)::value;
        if constexpr (npl <= 4) hipLaunchKernelGGL((k_score_segments_vec<npl>), grid, block, 0, stream, sa, g, (int)nw);   // (score_check: NPL <= 4)
    });
    HIPCHK(hipGetLastError());
}

int smcpp_score_windows_exact(smcpp_im *im, int c, long long window_bp, long long *n_windows, double *out) {
    API_BEGIN
    // the segment walk exists in the vectors form only (a matrix-form one would contract M x M per segment): asked first, so that the
    // refusal names the switch whatever else the matrix form would object to
    if (!im->score_form_vectors())
        throw std::runtime_error("score track: exact windows exist in the vectors form of the row walk only: set SMCPP_SCORE_FORM=vectors "
                                 "(one-population models prepared on the device, at most 256 hidden states)");
    const int nck = im->score_check(c);
    const long long nwin = window_count(im, c, window_bp, "score track", n_windows);
    score_cap(im->nder, nwin, "the windows");
    // the engine rows a boundary W, 2 W, .. < N cuts strictly inside; an item with nq boundaries owns nq + 1 slots
    const long long N = im->user_prefix[c][im->user_Ls[c]];
    im->walk_item_table(c, 0, N, window_bp, true, im->sx_items, im->sx_nslots);
    for (size_t k = 0; k < im->sx_items.size(); ++k) im->sx_items[k].seg += (long long)k;
    im->sx_nslots += (long long)im->sx_items.size();
    const long long nitems = (long long)im->sx_items.size(), nslots = im->sx_nslots;
    score_cap(3LL * im->nder, nslots, "the segments of the rows a window boundary cuts");
    // scratch: the parts per engine row and per segment + the parked block and the checkpoints of one wavefront at the least
    const size_t nd = (size_t)im->nder, MS = (size_t)64 * im->NPL;
    const size_t fixed = (size_t)3 * nd * ((size_t)im->Ls[c] + 1 + (size_t)nslots) * sizeof(double);
    const size_t per_wave = (size_t)SV_BLK * 4 * MS * sizeof(float) + (size_t)nck * MS * sizeof(double);
    if (nitems > 0 && fixed + per_wave > (1ull << 30))
        throw std::runtime_error("score track: the scratch of the exact windows (" + std::to_string(im->nder) + " directions x 3 parts x (" +
                                 std::to_string(im->Ls[c] + 1) + " engine rows + " + std::to_string(nslots) +
                                 " segments of cut rows)) exceeds the cap of 1 GiB: ask for a wider window");
    if (!out) return 0;
    im->score_rows(c, 0, 1, 1, 0, nck);                // every engine row -> d_sc_eng (the selection: column 0 alone, not used here)
    hipStream_t s = im->stream;
    long long nw = 0;
    if (nitems > 0) {
        nw = walk_waves(nitems, im->walk_slots(), per_wave, (1ull << 30) - fixed);
        if (opt().has(smcpp_opt::O_SCORE_WAVES)) nw = std::min(nw, std::max<long long>(1, opt().ll(smcpp_opt::O_SCORE_WAVES, 1)));
        im->score_segments_vec(c, nck, window_bp, nw);
    } else {
        im->d_sx_items.alloc(1);
        im->d_sx_seg.alloc(1);
    }
    im->sx_nitems = nitems; im->sx_nseg = nslots; im->sx_waves = (int)nw;
    if (nwin > 0) {                                    // (a contig without rows has no base pairs and no windows)
        const long long *EP = im->ll_epos_dev(c);
        im->d_sx_out.alloc((size_t)im->nder * nwin);
        hipLaunchKernelGGL(k_score_windows_exact, dim3((unsigned)ceil_div(nwin, 4)), dim3(256), 0, s, (long long)im->Ls[c], window_bp, nwin,
                           im->nder, EP, (const double *)im->d_sc_eng.p, (const LlItem *)im->d_sx_items.p, (int)nitems, nslots,
                           (const double *)im->d_sx_seg.p, im->d_sx_out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, im->d_sx_out.p, sizeof(double) * (size_t)im->nder * nwin, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    API_END
}
