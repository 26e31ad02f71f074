// engine_capi.hpp - part of the ONE translation unit engine.hip (included there, in order; not a standalone header):
// the C ABI of include/smcpp_engine.h.
// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
#define API_BEGIN try {
#define API_END                                                                    \
    return 0;                                                                      \
    }                                                                              \
    catch (const std::exception &e) { g_err = e.what(); return 1; }               \
    catch (...) { g_err = "unknown error"; return 1; }

extern "C" {

const char *smcpp_last_error(void) { return g_err.c_str(); }

int smcpp_create_onepop(int n, int n_contigs, const int *Ls, const int *const *obs, int n_hs, const double *hs,
                        double polarization_error, int device, smcpp_im **out) {
    API_BEGIN
    std::unique_ptr<smcpp_im> im(new smcpp_im());
    const int nn[1] = {n}, nna[1] = {2};
    im->build(1, nn, nna, n_contigs, Ls, obs, n_hs, hs, polarization_error, device);
    *out = im.release();
    API_END
}

int smcpp_create_twopop(int n1, int n2, int a1, int a2, int n_contigs, const int *Ls, const int *const *obs,
                        int n_hs, const double *hs, double polarization_error, int device, smcpp_im **out) {
    API_BEGIN
    if (a1 == 0 && a2 == 2) throw std::runtime_error("(0,2) not supported");
    if (a1 + a2 != 2) throw std::runtime_error("configuration not supported");
    std::unique_ptr<smcpp_im> im(new smcpp_im());
    const int nn[2] = {n1, n2}, nna[2] = {a1, a2};
    im->build(2, nn, nna, n_contigs, Ls, obs, n_hs, hs, polarization_error, device);
    *out = im.release();
    API_END
}

int smcpp_rccl_destroy(smcpp_im *im);
void smcpp_destroy(smcpp_im *im) { if (im && im->rccl) (void)smcpp_rccl_destroy(im); delete im; }

int smcpp_set_theta(smcpp_im *im, double v) { API_BEGIN im->params_fresh = false; im->theta = v; im->dirty = true; if (im->have_model) im->have_raw = false; API_END }
int smcpp_set_rho(smcpp_im *im, double v) { API_BEGIN im->params_fresh = false; im->rho = v; im->dirty = true; if (im->have_model) im->have_raw = false; API_END }
int smcpp_set_alpha(smcpp_im *im, double v) { API_BEGIN im->params_fresh = false; im->alpha = v; im->dirty = true; if (im->have_model) im->have_raw = false; API_END }

int smcpp_set_params(smcpp_im *im, int K, const double *a, const double *da, int nder, const double *s) {
    API_BEGIN
    if (K <= 0) throw std::runtime_error("empty parameter vector");
    for (int k = 0; k < K; ++k)
        if (!(a[k] > 0)) throw std::runtime_error("model pieces must be positive");
    if (nder > smcpp_host::MAXD) throw std::runtime_error("too many derivative directions (max 64)");
    im->model.a.assign(a, a + K);
    im->model.s.assign(s, s + K);
    im->nder = (da && nder > 0) ? nder : 0;
    im->model_da.clear();
    if (im->nder) im->model_da.assign(da, da + (size_t)K * nder);
    im->params_fresh = false;
    im->have_model = true;
    im->have_raw = false;
    im->dirty = true;
    API_END
}

int smcpp_set_params_twopop(smcpp_im *im, int Kd, const double *ad, const double *sd, const double *dad, int K1,
                            const double *a1, const double *s1, const double *da1, int K2, const double *a2,
                            const double *s2, const double *da2, double split, int nder) {
    API_BEGIN
    if (im->npop != 2) throw std::runtime_error("set_params_twopop on a one-population manager");
    if (Kd <= 0 || K1 <= 0 || K2 <= 0) throw std::runtime_error("empty parameter vector");
    if (!(split >= 0)) throw std::runtime_error("split time must be >= 0");
    if (nder > smcpp_host::MAXD) throw std::runtime_error("too many derivative directions (max 64)");
    auto chk = [](int K, const double *a) {
        for (int k = 0; k < K; ++k)
            if (!(a[k] > 0)) throw std::runtime_error("model pieces must be positive");
    };
    chk(Kd, ad); chk(K1, a1); chk(K2, a2);
    im->model.a.assign(ad, ad + Kd); im->model.s.assign(sd, sd + Kd);
    im->model_p1.a.assign(a1, a1 + K1); im->model_p1.s.assign(s1, s1 + K1);
    im->model_p2.a.assign(a2, a2 + K2); im->model_p2.s.assign(s2, s2 + K2);
    im->split = split;
    im->nder = nder > 0 ? nder : 0;
    im->model_da.clear(); im->model_da1.clear(); im->model_da2.clear();
    if (im->nder) {
        if (dad) im->model_da.assign(dad, dad + (size_t)Kd * nder);
        if (da1) im->model_da1.assign(da1, da1 + (size_t)K1 * nder);
        if (da2) im->model_da2.assign(da2, da2 + (size_t)K2 * nder);
    }
    im->params_fresh = false;
    im->have_model = true;
    im->have_raw = false;
    im->dirty = true;
    API_END
}

int smcpp_set_prep_mode(smcpp_im *im, int host) {
    API_BEGIN
    im->force_host_prep = host != 0;
    im->params_fresh = false;
    im->dirty = true;
    API_END
}

int smcpp_set_warm_start(smcpp_im *im, int on) {
    API_BEGIN
    im->warm_start = on != 0;
    if (!on) im->warm_valid = false;
    API_END
}

int smcpp_set_raw(smcpp_im *im, const double *pi, const double *T, int K, const int *keys, const double *E) {
    API_BEGIN
    const int M = im->M, kl = im->keylen;
    std::map<std::vector<int>, int> given;
    for (int k = 0; k < K; ++k) given[std::vector<int>(keys + (size_t)k * kl, keys + (size_t)(k + 1) * kl)] = k;
    std::vector<double> Enew((size_t)im->K * M);
    for (int k = 0; k < im->K; ++k) {
        std::vector<int> key(im->keys.begin() + (size_t)k * kl, im->keys.begin() + (size_t)(k + 1) * kl);
        auto it = given.find(key);
        if (it == given.end()) throw std::runtime_error("set_raw: an observed key has no emission vector");
        std::memcpy(&Enew[(size_t)k * M], E + (size_t)it->second * M, sizeof(double) * M);
    }
    im->pi.assign(pi, pi + M);
    im->T.assign(T, T + (size_t)M * M);
    im->E.swap(Enew);
    im->raw_keys.assign(keys, keys + (size_t)K * kl);
    im->raw_E.assign(E, E + (size_t)K * M);
    im->have_raw = true;
    im->E_on_dev = false;
    im->tgen_valid = false; im->dT_valid = true; im->T_lazy = false;
    im->dirty = true;
    im->nder = 0;
    API_END
}

int smcpp_estep(smcpp_im *im, int fb_only) {
    API_BEGIN
    (void)fb_only;   // accepted and ignored, as in the reference (hmm.cpp:45)
    im->estep();
    API_END
}

int smcpp_loglik(smcpp_im *im, double *out) {
    API_BEGIN
    std::memcpy(out, im->loglik.data(), sizeof(double) * im->n_contigs);    // 0 before the first E-step (hmm.cpp:11: ll(0.))
    API_END
}

static double dcs(const std::vector<double> &x) {   // doubly_compensated_summation, common.h:27-46
    if (x.empty()) return 0.0;
    double s = x[0], c = 0.0;
    for (size_t i = 1; i < x.size(); ++i) {
        const double y = c + x[i];
        const double u = x[i] - (y - c);
        const double t = y + s;
        const double v = y - (t - s);
        const double z = u + v;
        s = t + z;
        c = z - (s - t);
    }
    return s;
}

int smcpp_q(smcpp_im *im, double val[4], double *jac) {
    API_BEGIN
    const int M = im->M, K = im->K;
    if (!im->have_raw) im->prepare_params();   // Q() does do_dirty_work() first (inference_manager.cpp:119)
    im->q_route = smcpp_im::Q_ROUTE_NONE;
    if (im->q_device(val, jac)) { im->q_route = smcpp_im::Q_ROUTE_DEVICE; return 0; }
    im->q_route = smcpp_im::Q_ROUTE_HOST;
    im->sync_host_E();
    im->ensure_dT();
    if ((int)im->pi.size() != M) throw std::runtime_error("parameters are not set");
    const int nder = im->have_raw ? 0 : im->nder;
    if (jac) for (int i = 0; i < 4 * nder; ++i) jac[i] = 0.0;
    for (int i = 0; i < 4; ++i) val[i] = 0.0;
    im->ensure_T();
    std::vector<double> logpi(M), logT((size_t)M * M), logE((size_t)K * M);
    for (int i = 0; i < M; ++i) logpi[i] = std::log(im->pi[i]);
    for (size_t i = 0; i < logT.size(); ++i) logT[i] = std::log(im->T[i]);
    std::vector<unsigned char> bad(K, 0);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < M; ++i) {
            if (im->E[(size_t)k * M + i] <= 0.0) bad[k] = 1;
            logE[(size_t)k * M + i] = std::log(im->E[(size_t)k * M + i]);
        }
    // d/d(seed) of sum w log x = sum (w / x) dx  (forward-mode derivatives of hmm.cpp:161-185)
    auto add_jac = [&](int term, const double *w, const double *x, const double *dx, size_t cnt) {
        if (!jac || nder == 0) return;
        for (size_t i = 0; i < cnt; ++i) {
            const double f = w[i] / x[i];
            for (int d = 0; d < nder; ++d) jac[term * nder + d] += f * dx[i * nder + d];
        }
    };
    if (im->have_reduced) {
        // statistics already summed over every rank's contigs: every global key contributes, also those no contig of
        // this rank holds (their emission vectors come from the same preparation, see prepare_params)
        const double *g0 = &im->g_stats[1], *xs = g0 + M, *gs = xs + (size_t)M * M;
        const int Kg = (int)(im->gkeys.size() / im->keylen), kl = im->keylen;
        im->global_emissions();
        for (int i = 0; i < M; ++i) val[0] += logpi[i] * g0[i];
        add_jac(0, g0, im->pi.data(), im->dpi.data(), M);
        std::vector<double> b0, b1;
        bool inf0 = false, inf1 = false;
        for (int kg = 0; kg < Kg; ++kg) {
            const double *e = &im->Eg[(size_t)kg * M], *g = gs + (size_t)kg * M;
            int nb = 0;
            for (int p = 0; p < im->npop; ++p) nb += im->gkeys[(size_t)kg * kl + 3 * p + 2];
            bool any = false, nan = false, nonpos = false;
            for (int i = 0; i < M; ++i) { any = any || g[i] != 0.0; nan = nan || std::isnan(e[i]); nonpos = nonpos || e[i] <= 0.0; }
            if (!any) continue;                          // no contig anywhere holds the key (hmm.cpp:166-181 skips it too)
            if (nan) throw std::runtime_error("Q on all-reduced statistics: no emission vector for a key that another "
                                              "rank's contigs hold (set_raw must supply every global key)");
            if (nonpos) { (nb > 0 ? inf1 : inf0) = true; continue; }
            auto &b = nb > 0 ? b1 : b0;
            for (int i = 0; i < M; ++i) b.push_back(std::log(e[i]) * g[i]);
            if (nder) {
                if (im->dEg.empty()) throw std::runtime_error("Q gradient on all-reduced statistics needs model parameters (set_params)");
                add_jac(nb > 0 ? 2 : 1, g, e, &im->dEg[(size_t)kg * M * nder], M);
            }
        }
        val[1] = inf0 ? -INFINITY : dcs(b0);
        val[2] = inf1 ? -INFINITY : dcs(b1);
        std::vector<double> es((size_t)M * M);
        for (int j = 0; j < M; ++j)
            for (int i = 0; i < M; ++i) es[(size_t)j * M + i] = logT[(size_t)i * M + j] * xs[(size_t)i * M + j];
        val[3] = dcs(es);
        add_jac(3, xs, im->T.data(), im->dT.data(), (size_t)M * M);
        return 0;
    }
    im->fetch_stats();
    for (int c = 0; c < im->n_contigs; ++c) {
        double q0 = 0.0;
        for (int i = 0; i < M; ++i) q0 += logpi[i] * im->h_gamma0[(size_t)c * M + i];
        val[0] += q0;
        add_jac(0, &im->h_gamma0[(size_t)c * M], im->pi.data(), im->dpi.data(), M);
        std::vector<double> b0, b1;
        bool inf0 = false, inf1 = false;
        for (int k = 0; k < K; ++k) {
            if (!im->present[(size_t)c * K + k]) continue;
            if (bad[k]) { (im->key_nbpos[k] ? inf1 : inf0) = true; continue; }
            auto &b = im->key_nbpos[k] ? b1 : b0;
            for (int i = 0; i < M; ++i)
                b.push_back(logE[(size_t)k * M + i] * im->h_gsum[((size_t)c * K + k) * M + i]);
            add_jac(im->key_nbpos[k] ? 2 : 1, &im->h_gsum[((size_t)c * K + k) * M], &im->E[(size_t)k * M],
                    nder ? &im->dE[(size_t)k * M * nder] : nullptr, M);
        }
        val[1] += inf0 ? -INFINITY : dcs(b0);
        val[2] += inf1 ? -INFINITY : dcs(b1);
        std::vector<double> es((size_t)M * M);
        const double *xs = &im->h_xisum[(size_t)c * M * M];
        for (int j = 0; j < M; ++j)
            for (int i = 0; i < M; ++i) es[(size_t)j * M + i] = logT[(size_t)i * M + j] * xs[(size_t)i * M + j];
        val[3] += dcs(es);
        add_jac(3, xs, im->T.data(), im->dT.data(), (size_t)M * M);
    }
    API_END
}

int smcpp_set_save_gamma(smcpp_im *im, int on) { API_BEGIN im->save_gamma = on != 0; API_END }
int smcpp_get_save_gamma(smcpp_im *im) { return im->save_gamma ? 1 : 0; }
int smcpp_num_states(smcpp_im *im) { return im->M; }
int smcpp_num_contigs(smcpp_im *im) { return im->n_contigs; }
int smcpp_num_keys(smcpp_im *im) { return im->K; }
int smcpp_key_len(smcpp_im *im) { return im->keylen; }

int smcpp_get_hidden_states(smcpp_im *im, double *hs) {
    API_BEGIN std::memcpy(hs, im->hs.data(), sizeof(double) * im->hs.size()); API_END
}
int smcpp_set_hidden_states(smcpp_im *im, int n_hs, const double *hs) {
    API_BEGIN
    if (n_hs != (int)im->hs.size()) throw std::runtime_error("hidden states must be same size");
    im->hs.assign(hs, hs + n_hs);
    im->update_pi_default();
    im->twopop_prep.reset();
    if (!im->estep_done) im->stats_on_host = false;
    if (im->qdev) im->qdev->stats_ready = false;      // the pre-E-step statistics are span_sum * pi_default: restage them
    im->dirty = true;
    im->params_fresh = false;
    if (im->have_model) im->have_raw = false;
    API_END
}
int smcpp_get_keys(smcpp_im *im, int *keys) {
    API_BEGIN std::memcpy(keys, im->keys.data(), sizeof(int) * im->keys.size()); API_END
}

int smcpp_get_xisum(smcpp_im *im, int c, double *out) {
    API_BEGIN
    if (c < 0 || c >= im->n_contigs) throw std::runtime_error("contig index out of range");
    im->fetch_stats();
    std::memcpy(out, &im->h_xisum[(size_t)c * im->M * im->M], sizeof(double) * im->M * im->M);
    API_END
}

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
    if (nq < 0 || nq > 8) throw std::runtime_error("posterior summary: between 0 and 8 quantile levels");
    if (nq > 0 && !q) throw std::runtime_error("posterior summary: quantile levels are missing");
    PostLevels lv;
    lv.nq = nq;
    for (int k = 0; k < 8; ++k) lv.q[k] = 2.0;
    for (int k = 0; k < nq; ++k) {
        if (!(q[k] > 0.0 && q[k] < 1.0)) throw std::runtime_error("posterior summary: a quantile level must lie in (0, 1)");
        lv.q[k] = q[k];
    }
    const int M = im->M;
    if (weights)
        for (int i = 0; i < M; ++i)
            if (!std::isfinite(weights[i])) throw std::runtime_error("posterior summary: weight " + std::to_string(i) + " is not finite");
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
    if (window_bp < 1) throw std::runtime_error("posterior windows: window_bp < 1");
    const std::vector<long long> &P = im->user_prefix[c];
    const long long L = im->user_Ls[c];
    const long long nwin = (P[L] + window_bp - 1) / window_bp;
    if (n_windows) *n_windows = nwin;
    if (!out) return 0;
    if (nwin > (1LL << 31) - 1 - PW_WPB) throw std::runtime_error("posterior windows: too many windows for one launch (widen the window)");
    const smcpp_im::PostSource src = im->post_source(c);
    hipStream_t s = im->stream;
    const int M = im->M, Mp = im->Mp;
    if (im->d_user_prefix.size() != (size_t)im->n_contigs) im->d_user_prefix.resize(im->n_contigs);
    if (!im->d_user_prefix[c].p) {
        im->d_user_prefix[c].upload(P, s);             // (P is a member: it outlives the copy)
        HIPCHK(hipStreamSynchronize(s));
    }
    // the column sums of every row, by the kernel that serves smcpp_posterior_summary: p is the same number in every product
    PostSel all;
    all.start = 0; all.step = 1; all.ncols = L + 1;
    PostLevels none;
    none.nq = 0;
    for (int k = 0; k < 8; ++k) none.q[k] = 2.0;
    im->d_post_colsum.alloc((size_t)L + 1);
    hipLaunchKernelGGL(k_post_summary, dim3((unsigned)ceil_div(all.ncols, PS_TL)), dim3(256), 0, s, M, Mp, all, src.rows, src.g0,
                       (const double *)nullptr, none, im->d_post_colsum.p, (int *)nullptr, (double *)nullptr, (int *)nullptr);
    HIPCHK(hipGetLastError());
    im->d_post_out.alloc((size_t)M * nwin);
    hipLaunchKernelGGL(k_post_windows, dim3((unsigned)ceil_div(nwin, PW_WPB), (unsigned)ceil_div(M, 64)), dim3(256), 0, s, M, Mp, L,
                       window_bp, nwin, (const long long *)im->d_user_prefix[c].p, src.rows, (const double *)im->d_post_colsum.p,
                       im->d_post_out.p);
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
    if (!ss_active && !ss_generators_only())
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
    d_pt_gen.upload(ss_gen, stream);                   // (ss_gen is a member: it outlives the copy)
    SsArgs sa = SsArgs();
    sa.M = M; sa.Mp = Mp;
    const double *gd = d_pt_gen.p;
    sa.f_dc = gd; sa.f_g = gd + MS; sa.f_cg = gd + 2 * MS; sa.f_b = gd + 3 * MS; sa.f_a = gd + 4 * MS; sa.f_d = gd + 5 * MS;
    sa.b_dc = gd + 6 * MS; sa.b_g = gd + 7 * MS; sa.b_b = gd + 8 * MS; sa.b_a = gd + 9 * MS;
    sa.c0 = ss_c0;
    PtArgs pa;
    pa.M = M; pa.Mp = Mp; pa.L = Le; pa.base = contig_base[c];
    int smax = 1;                                      // the contig's longest engine row
    for (int i = 1; i <= Le; ++i) {
        const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
        if (ri.gid >= 0) smax = std::max(smax, groups[ri.gid].span);
    }
    pa.nck = (smax + PT_BLK - 1) / PT_BLK - 1;
    // one wavefront per row, persistent; fewer of them where the scratch of a wavefront is large (many states per lane, or the
    // checkpoints of a very long row): at most 1 GiB in all
    const size_t per_wave = (size_t)PT_BLK * 3 * MS * sizeof(float) + (size_t)pa.nck * MS * sizeof(double);
    const long long want = std::min<long long>(Le, NPL >= 8 ? 1024 : 4096);
    const int nw = (int)std::max<long long>(1, std::min<long long>(want, (long long)((1ull << 30) / per_wave)));
    d_pt_park.alloc((size_t)nw * PT_BLK * 3 * MS);
    d_pt_ckpt.alloc(std::max<size_t>(1, (size_t)nw * pa.nck * MS));
    d_pt_eng.alloc((size_t)3 * (Le + 1));
    pa.rowinfo = d_rowinfo.p; pa.g_span = d_g_span.p; pa.E = d_E.p; pa.alpha = d_alpha.p; pa.beta = d_beta.p;
    pa.park = d_pt_park.p; pa.ckpt = d_pt_ckpt.p; pa.out = d_pt_eng.p;
    pt_waves = nw;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    switch (NPL) {
#define PT_(x) case x: hipLaunchKernelGGL((k_post_transitions<x>), grid, block, 0, stream, sa, pa, nw); break;
        PT_(1) PT_(2) PT_(3) PT_(4) PT_(8)
        default: PT_(16)
#undef PT_
    }
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
    if (window_bp < 1) throw std::runtime_error("posterior transition windows: window_bp < 1");
    im->post_transitions_check();
    const std::vector<long long> &P = im->user_prefix[c];
    const long long L = im->user_Ls[c];
    const long long nwin = (P[L] + window_bp - 1) / window_bp;
    if (n_windows) *n_windows = nwin;
    if (!out) return 0;
    if (nwin > 4 * ((1LL << 31) - 1)) throw std::runtime_error("posterior transition windows: too many windows for one launch (widen the window)");
    const double *v = im->post_transitions(c, 0, 1, L + 1);
    hipStream_t s = im->stream;
    if (im->d_user_prefix.size() != (size_t)im->n_contigs) im->d_user_prefix.resize(im->n_contigs);
    if (!im->d_user_prefix[c].p) {
        im->d_user_prefix[c].upload(P, s);             // (P is a member: it outlives the copy)
        HIPCHK(hipStreamSynchronize(s));
    }
    im->d_post_out.alloc((size_t)3 * nwin);
    hipLaunchKernelGGL(k_post_transition_windows, dim3((unsigned)ceil_div(nwin, 4)), dim3(256), 0, s, L, window_bp, nwin,
                       (const long long *)im->d_user_prefix[c].p, v, im->d_post_out.p);
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
    int smax = 1;                                      // the contig's longest engine row
    for (int i = 1; i <= Le; ++i) {
        const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
        if (ri.gid >= 0) smax = std::max(smax, groups[ri.gid].span);
    }
    PpArgs pa;
    pa.nck = (smax + PP_BLK - 1) / PP_BLK - 1;
    // paths per wavefront: as few as fill the wavefront slots (a batch shares the forward walk, but its paths run one behind the other)
    const long long slots = NPL >= 8 ? 1024 : 4096;
    long long batch = opt().has(smcpp_opt::O_PATH_BATCH) ? opt().ll(smcpp_opt::O_PATH_BATCH, 1) : (npaths + slots - 1) / slots;
    batch = std::max<long long>(1, std::min<long long>(64, batch));
    const long long nbatches = (npaths + batch - 1) / batch;
    // scratch per wavefront: one block of parked vectors + the checkpoints of the longest row; at most 1 GiB in all
    const size_t per_wave = (size_t)PP_BLK * MS * sizeof(float) + (size_t)pa.nck * MS * sizeof(double);
    if (per_wave > (1ull << 30))
        throw std::runtime_error("posterior paths: the checkpoints of a row of " + std::to_string(smax) + " positions exceed the scratch "
                                 "cap of 1 GiB");
    const int nw = (int)std::max<long long>(1, std::min<long long>(std::min(nbatches, slots), (long long)((1ull << 30) / per_wave)));
    const int *first = want_rows ? piece_first_dev(c) : nullptr;
    ensure_T();
    if ((int)T.size() != M * M) throw std::runtime_error("posterior paths: the transition matrix is missing");
    std::vector<double> TT((size_t)(M + 1) * MS, 0.0);
    for (int j = 0; j < M; ++j)
        for (int i = 0; i < M; ++i) TT[(size_t)j * MS + i] = T[(size_t)i * M + j];
    for (int i = 0; i < M; ++i) TT[(size_t)M * MS + i] = 1.0;
    d_pp_TT.upload(TT, stream);
    d_pt_gen.upload(ss_gen, stream);                   // (ss_gen is a member: it outlives the copy)
    SsArgs sa = SsArgs();
    sa.M = M; sa.Mp = Mp;
    const double *gd = d_pt_gen.p;
    sa.f_dc = gd; sa.f_g = gd + MS; sa.f_cg = gd + 2 * MS; sa.f_b = gd + 3 * MS; sa.f_a = gd + 4 * MS; sa.f_d = gd + 5 * MS;
    sa.b_dc = gd + 6 * MS; sa.b_g = gd + 7 * MS; sa.b_b = gd + 8 * MS; sa.b_a = gd + 9 * MS;
    sa.c0 = ss_c0;
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
    switch (NPL) {
#define PP_(x) case x: hipLaunchKernelGGL((k_post_paths<x>), grid, block, 0, stream, sa, pa, nw); break;
        PP_(1) PP_(2) PP_(3) PP_(4) PP_(8)
        default: PP_(16)
#undef PP_
    }
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
    const long long N = im->user_prefix[c][im->user_Ls[c]];
    if (pos0 < 0) throw std::runtime_error("posterior paths: pos0 < 0");
    if (pos1 > N + 1) throw std::runtime_error("posterior paths: pos1 > P_L + 1 (the contig has " + std::to_string(N + 1) + " positions)");
    if (pos0 >= pos1) throw std::runtime_error("posterior paths: empty window of positions (pos0 >= pos1)");
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
    const long long slots = NPL >= 8 ? 1024 : 4096;
    const int nw = (int)std::min(units, slots);
    im->sim_waves = nw; im->sim_units = units; im->sim_events = 0;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    switch (NPL) {
#define SIM_(x) case x: hipLaunchKernelGGL((k_simulate<x>), grid, block, 0, s, sa, nw); break;
        SIM_(1) SIM_(2) SIM_(3) SIM_(4) SIM_(8)
        default: SIM_(16)
#undef SIM_
    }
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
    const size_t per_wave = (size_t)PQ_BLK * MS * sizeof(float) + (size_t)((pq_smax + PQ_BLK - 1) / PQ_BLK - 1) * MS * sizeof(double);
    if (per_wave > (1ull << 30))
        throw std::runtime_error("posterior positions: the checkpoints of a row of " + std::to_string(pq_smax) + " positions exceed the "
                                 "scratch cap of 1 GiB");
    if (extra_bytes > (1ull << 30))
        throw std::runtime_error("posterior positions: the segment sums of the cut rows (" + std::to_string(pq_nseg) + " vectors) exceed "
                                 "the scratch cap of 1 GiB (widen the window)");
}

// the column sums of every caller's row, by the kernel that serves smcpp_posterior_summary: p is the same number in every product
const double *smcpp_im::post_colsum(int c, const PostSource &src) {
    PostSel all;
    all.start = 0; all.step = 1; all.ncols = (long long)user_Ls[c] + 1;
    PostLevels none;
    none.nq = 0;
    for (int k = 0; k < 8; ++k) none.q[k] = 2.0;
    d_pq_colsum.alloc((size_t)all.ncols);
    hipLaunchKernelGGL(k_post_summary, dim3((unsigned)ceil_div(all.ncols, PS_TL)), dim3(256), 0, stream, M, Mp, all, src.rows, src.g0,
                       (const double *)nullptr, none, d_pq_colsum.p, (int *)nullptr, (double *)nullptr, (int *)nullptr);
    HIPCHK(hipGetLastError());
    return d_pq_colsum.p;
}

// Launches k_post_positions over pq_items (not empty) with sink `kind`; the sink's fields of pa are the caller's, the rest is set here.
// The arguments have been checked.
void smcpp_im::post_positions_launch(int c, int kind, PqArgs &pa) {
    const int MS = 64 * NPL;
    d_pt_gen.upload(ss_gen, stream);                   // (ss_gen is a member: it outlives the copy)
    SsArgs sa = SsArgs();
    sa.M = M; sa.Mp = Mp;
    const double *gd = d_pt_gen.p;
    sa.f_dc = gd; sa.f_g = gd + MS; sa.f_cg = gd + 2 * MS; sa.f_b = gd + 3 * MS; sa.f_a = gd + 4 * MS; sa.f_d = gd + 5 * MS;
    sa.b_dc = gd + 6 * MS; sa.b_g = gd + 7 * MS; sa.b_b = gd + 8 * MS; sa.b_a = gd + 9 * MS;
    sa.c0 = ss_c0;
    pa.M = M; pa.Mp = Mp; pa.base = contig_base[c];
    pa.nck = (pq_smax + PQ_BLK - 1) / PQ_BLK - 1;
    pa.nitems = (int)pq_items.size();
    // one wavefront per item, persistent; fewer of them where the scratch of a wavefront is large: at most 1 GiB in all
    const size_t per_wave = (size_t)PQ_BLK * MS * sizeof(float) + (size_t)pa.nck * MS * sizeof(double);
    const long long want = std::min<long long>(pa.nitems, NPL >= 8 ? 1024 : 4096);
    const int nw = (int)std::max<long long>(1, std::min<long long>(want, (long long)((1ull << 30) / per_wave)));
    d_pq_items.upload(pq_items, stream);               // (a member: it outlives the copy)
    d_pq_park.alloc((size_t)nw * PQ_BLK * MS);
    d_pq_ckpt.alloc(std::max<size_t>(1, (size_t)nw * pa.nck * MS));
    pa.rowinfo = d_rowinfo.p; pa.g_span = d_g_span.p; pa.E = d_E.p; pa.alpha = d_alpha.p; pa.beta = d_beta.p;
    pa.items = d_pq_items.p; pa.park = d_pq_park.p; pa.ckpt = d_pq_ckpt.p;
    pq_waves = nw;
    const dim3 grid(ceil_div(nw, 4)), block(256);
#define PQ_(x, S) case x: hipLaunchKernelGGL((k_post_positions<x, S>), grid, block, 0, stream, sa, pa, nw); break;
#define PQ_ALL(S) switch (NPL) { PQ_(1, S) PQ_(2, S) PQ_(3, S) PQ_(4, S) PQ_(8, S) default: PQ_(16, S) }
    if (kind == 0) PQ_ALL(PqColumns)
    else if (kind == 1) PQ_ALL(PqSummary)
    else PQ_ALL(PqSegments)
#undef PQ_ALL
#undef PQ_
    HIPCHK(hipGetLastError());
}

// pos0 / pos1 / step of a grid over the positions 0 .. N of contig c -> the number of grid positions
static long long post_positions_check_grid(smcpp_im *im, int c, long long pos0, long long pos1, long long step) {
    const long long N = im->user_prefix[c][im->user_Ls[c]];
    if (pos0 < 0) throw std::runtime_error("posterior positions: pos0 < 0");
    if (pos1 > N + 1) throw std::runtime_error("posterior positions: pos1 > P_L + 1 (the contig has " + std::to_string(N + 1) + " positions)");
    if (pos0 >= pos1) throw std::runtime_error("posterior positions: empty grid (pos0 >= pos1)");
    if (step < 1) throw std::runtime_error("posterior positions: step < 1");
    return (pos1 - pos0 + step - 1) / step;
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
    const long long npos = post_positions_check_grid(im, c, pos0, pos1, step);
    post_positions_cap(im->M, npos, "the columns");
    im->post_positions_grid(c, pos0, pos1, step);
    im->post_positions_scratch_check(0);
    if (!out) return 0;
    const smcpp_im::PostSource src = im->post_source(c);
    PqArgs pa = PqArgs();
    pa.rows = src.rows; pa.g0 = src.g0; pa.colsum = im->post_colsum(c, src);
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
    const long long npos = post_positions_check_grid(im, c, pos0, pos1, step);
    if (nq < 0 || nq > 8) throw std::runtime_error("posterior position summary: between 0 and 8 quantile levels");
    if (nq > 0 && !q) throw std::runtime_error("posterior position summary: quantile levels are missing");
    PqArgs pa = PqArgs();
    pa.lv.nq = nq;
    for (int k = 0; k < 8; ++k) pa.lv.q[k] = 2.0;
    for (int k = 0; k < nq; ++k) {
        if (!(q[k] > 0.0 && q[k] < 1.0)) throw std::runtime_error("posterior position summary: a quantile level must lie in (0, 1)");
        pa.lv.q[k] = q[k];
    }
    const int M = im->M;
    if (weights)
        for (int i = 0; i < M; ++i)
            if (!std::isfinite(weights[i])) throw std::runtime_error("posterior position summary: weight " + std::to_string(i) + " is not finite");
    post_positions_cap(std::max(1, nq), npos, "the summaries");
    im->post_positions_grid(c, pos0, pos1, step);
    im->post_positions_scratch_check(0);
    const bool want_mean = weights && mean, want_q = nq > 0 && qstate;
    if (!argmax && !want_mean && !want_q) return 0;
    const smcpp_im::PostSource src = im->post_source(c);
    hipStream_t s = im->stream;
    pa.rows = src.rows; pa.g0 = src.g0; pa.colsum = im->post_colsum(c, src);
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
    if (window_bp < 1) throw std::runtime_error("posterior windows: window_bp < 1");
    im->post_transitions_check();
    const std::vector<long long> &P = im->user_prefix[c];
    const long long L = im->user_Ls[c];
    const long long nwin = (P[L] + window_bp - 1) / window_bp;
    if (n_windows) *n_windows = nwin;
    if (!out) return 0;
    post_positions_cap(im->M, nwin, "the windows");
    im->post_positions_segments(c, window_bp);
    const int M = im->M, Mp = im->Mp, MS = 64 * im->NPL;
    im->post_positions_scratch_check((size_t)im->pq_nseg * MS * sizeof(double));
    const smcpp_im::PostSource src = im->post_source(c);
    hipStream_t s = im->stream;
    if (im->d_user_prefix.size() != (size_t)im->n_contigs) im->d_user_prefix.resize(im->n_contigs);
    if (!im->d_user_prefix[c].p) {
        im->d_user_prefix[c].upload(P, s);             // (P is a member: it outlives the copy)
        HIPCHK(hipStreamSynchronize(s));
    }
    const double *colsum = im->post_colsum(c, src);
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
                       window_bp, nwin, (const long long *)im->d_user_prefix[c].p, src.rows, colsum, (const PqItem *)im->d_pq_items.p,
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
    if (!split_spans) {
        if (d_user_prefix.size() != (size_t)n_contigs) d_user_prefix.resize(n_contigs);
        if (!d_user_prefix[c].p) {
            d_user_prefix[c].upload(user_prefix[c], stream);               // (a member: it outlives the copy)
            HIPCHK(hipStreamSynchronize(stream));
        }
        return d_user_prefix[c].p;
    }
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
void smcpp_im::ll_table(int c, long long pos0, long long pos1, long long step, bool windows) {
    const int Le = Ls[c];
    ll_items.clear();
    ll_nslots = 0;
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
                ll_items.push_back(LlItem{q0, g, windows ? ll_nslots : (g - pos0) / step, i, nq});
                ll_nslots += nq;
            }
        }
        q0 = end;
    }
}

void smcpp_im::ll_walk(int c, long long step, double *slots) {
    const int MS = 64 * NPL;
    d_ll_gen.upload(ss_gen, stream);                   // (ss_gen is a member: it outlives the copy)
    SsArgs sa = SsArgs();
    sa.M = M; sa.Mp = Mp;
    const double *gd = d_ll_gen.p;
    sa.f_dc = gd; sa.f_g = gd + MS; sa.f_cg = gd + 2 * MS; sa.f_b = gd + 3 * MS; sa.f_a = gd + 4 * MS; sa.f_d = gd + 5 * MS;
    sa.b_dc = gd + 6 * MS; sa.b_g = gd + 7 * MS; sa.b_b = gd + 8 * MS; sa.b_a = gd + 9 * MS;
    sa.c0 = ss_c0;
    LlArgs la = LlArgs();
    la.M = M; la.Mp = Mp; la.nitems = (int)ll_items.size(); la.base = contig_base[c];
    la.rowinfo = d_rowinfo.p; la.g_span = d_g_span.p; la.E = d_E.p; la.alpha = d_alpha.p; la.logc = d_logc.p; la.pre = d_ll_pre.p;
    d_ll_items.upload(ll_items, stream);               // (a member: it outlives the copy)
    d_ll_ratio.alloc((size_t)la.nitems);
    la.items = d_ll_items.p; la.step = step; la.out = slots; la.ratio = d_ll_ratio.p;
    // one wavefront per item, persistent: as many as there are wavefront slots, or as SMCPP_LL_WAVES allows
    long long nw = std::min<long long>(la.nitems, NPL >= 8 ? 1024 : 4096);
    if (opt().has(smcpp_opt::O_LL_WAVES)) nw = std::min(nw, std::max<long long>(1, opt().ll(smcpp_opt::O_LL_WAVES, 1)));
    ll_waves = (int)nw;
    const dim3 grid(ceil_div(nw, 4)), block(256);
    switch (NPL) {
#define LL_(x) case x: hipLaunchKernelGGL((k_ll_walk<x>), grid, block, 0, stream, sa, la, (int)nw); break;
        LL_(1) LL_(2) LL_(3) LL_(4) LL_(8)
        default: LL_(16)
#undef LL_
    }
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
    const long long N = im->user_prefix[c][im->user_Ls[c]];
    if (pos0 < 0) throw std::runtime_error("loglik track: pos0 < 0");
    if (pos1 > N + 1) throw std::runtime_error("loglik track: pos1 > P_L + 1 (the contig has " + std::to_string(N + 1) + " positions)");
    if (pos0 >= pos1) throw std::runtime_error("loglik track: empty grid (pos0 >= pos1)");
    if (step < 1) throw std::runtime_error("loglik track: step < 1");
    const long long npos = (pos1 - pos0 + step - 1) / step;
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
    if (window_bp < 1) throw std::runtime_error("loglik track: window_bp < 1");
    const long long N = im->user_prefix[c][im->user_Ls[c]];
    const long long nwin = (N + window_bp - 1) / window_bp;
    if (n_windows) *n_windows = nwin;
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
    if (M > 64 || NPL != 1)
        throw std::runtime_error("score track: more than 64 hidden states (" + std::to_string(M) + "): the kernel keeps one column of the "
                                 "M x M accumulator per lane and exists at one state per lane only");
    int smax = 1;                                     // the contig's longest engine row
    for (int i = 1; i <= Ls[c]; ++i) {
        const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
        if (ri.gid >= 0) smax = std::max(smax, groups[ri.gid].span);
    }
    const int nck = (smax + SC_BLK - 1) / SC_BLK - 1;
    // scratch: the three parts of every direction per engine row + one wavefront's checkpoints at the least
    const size_t bytes = ((size_t)3 * nder * ((size_t)Ls[c] + 1) + (size_t)nck * 64) * sizeof(double);
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
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<double> Ep, dEp, em, dem;
        dprep->fetch(Ep, dEp, em, dem, false);           // (the table and its Jacobian alone)
        dprep->check_flags();
        if (!have_global) { Eloc.swap(Ep); dEloc.swap(dEp); }
        else {
            Eloc.assign((size_t)K * M, 0.0);
            dEloc.assign((size_t)K * M * nder, 0.0);
            for (int k = 0; k < K; ++k) {
                const int kg = local_to_global[k];
                std::memcpy(&Eloc[(size_t)k * M], &Ep[(size_t)kg * M], sizeof(double) * M);
                std::memcpy(&dEloc[(size_t)k * M * nder], &dEp[(size_t)kg * M * nder], sizeof(double) * M * nder);
            }
        }
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

// The parts (parts != 0: [3][nder][ncols]) or the total ([nder][ncols]) of caller's rows start, start + step, .. of contig c, on the
// device, on `stream`.  The arguments have been checked (score_check -> nck, the caps).
const double *smcpp_im::score_rows(int c, long long start, long long step, long long ncols, int parts, int nck) {
    HIPCHK(hipSetDevice(device));
    score_tables();
    const int Le = Ls[c];
    const int *first = piece_first_dev(c);
    d_pt_gen.upload(ss_gen, stream);                   // (the transition products' copy of the generators; ss_gen is a member: it outlives the copy)
    SsArgs sa = SsArgs();
    sa.M = M; sa.Mp = Mp;
    const double *gd = d_pt_gen.p;
    sa.f_dc = gd; sa.f_g = gd + 64; sa.f_cg = gd + 2 * 64; sa.f_b = gd + 3 * 64; sa.f_a = gd + 4 * 64; sa.f_d = gd + 5 * 64;
    sa.b_dc = gd + 6 * 64; sa.b_g = gd + 7 * 64; sa.b_b = gd + 8 * 64; sa.b_a = gd + 9 * 64;
    sa.c0 = ss_c0;
    ScArgs a = ScArgs();
    a.M = M; a.Mp = Mp; a.L = Le; a.nck = nck; a.nder = nder; a.base = contig_base[c];
    // one wavefront per engine row, persistent: a workgroup's parked vectors fill a CU's LDS, so 4 wavefronts per CU are resident;
    // fewer where SMCPP_SCORE_WAVES says so or the checkpoints of a very long row would pass 1 GiB with the parts
    long long nw = std::max<long long>(1, std::min<long long>(Le, 1024));      // (a contig without rows: wavefront 0 writes column 0)
    if (opt().has(smcpp_opt::O_SCORE_WAVES)) nw = std::min(nw, std::max<long long>(1, opt().ll(smcpp_opt::O_SCORE_WAVES, 1)));
    if (nck > 0) {
        const size_t left = (1ull << 30) - (size_t)3 * nder * ((size_t)Le + 1) * sizeof(double);
        nw = std::max<long long>(1, std::min<long long>(nw, (long long)(left / ((size_t)nck * 64 * sizeof(double)))));
    }
    d_sc_ckpt.alloc(std::max<size_t>(1, (size_t)nw * nck * 64));
    d_sc_eng.alloc((size_t)3 * nder * ((size_t)Le + 1));
    a.rowinfo = d_rowinfo.p; a.g_span = d_g_span.p; a.E = d_E.p; a.alpha = d_alpha.p; a.beta = d_beta.p;
    a.gamma0 = d_gamma0.p + (size_t)c * Mp;
    a.Gpi = d_sc_tab.p; a.dT = a.Gpi + (size_t)nder * 64; a.GE = a.dT + (size_t)nder * 64 * 64;
    a.ckpt = d_sc_ckpt.p; a.out = d_sc_eng.p;
    sc_waves = (int)nw; sc_items = Le;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_score_rows), hipFuncAttributeMaxDynamicSharedMemorySize, SC_LDS_BYTES));
    hipLaunchKernelGGL(k_score_rows, dim3((unsigned)ceil_div(nw, 4)), dim3(256), SC_LDS_BYTES, stream, sa, a, (int)nw);
    HIPCHK(hipGetLastError());
    PostSel sel;
    sel.start = start; sel.step = step; sel.ncols = ncols;
    d_sc_sel.alloc((size_t)(parts ? 3 : 1) * nder * ncols);
    hipLaunchKernelGGL(k_score_select, dim3((unsigned)ceil_div(ncols * nder, 256)), dim3(256), 0, stream, sel, (long long)Le, nder, parts,
                       first, (const double *)d_sc_eng.p, d_sc_sel.p);
    HIPCHK(hipGetLastError());
    return d_sc_sel.p;
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
    if (window_bp < 1) throw std::runtime_error("score track: window_bp < 1");
    const std::vector<long long> &P = im->user_prefix[c];
    const long long L = im->user_Ls[c];
    const long long nwin = (P[L] + window_bp - 1) / window_bp;
    if (n_windows) *n_windows = nwin;
    score_cap(im->nder, nwin, "the windows");
    if (!out) return 0;
    const double *v = im->score_rows(c, 0, 1, L + 1, 0, nck);
    hipStream_t s = im->stream;
    if (im->d_user_prefix.size() != (size_t)im->n_contigs) im->d_user_prefix.resize(im->n_contigs);
    if (!im->d_user_prefix[c].p) {
        im->d_user_prefix[c].upload(P, s);             // (P is a member: it outlives the copy)
        HIPCHK(hipStreamSynchronize(s));
    }
    if (nwin > 0) {                                    // (a contig without rows has no base pairs and no windows)
        im->d_sc_out.alloc((size_t)im->nder * nwin);
        hipLaunchKernelGGL(k_score_windows, dim3((unsigned)ceil_div(nwin, 4)), dim3(256), 0, s, L, window_bp, nwin, im->nder,
                           (const long long *)im->d_user_prefix[c].p, v, im->d_sc_out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, im->d_sc_out.p, sizeof(double) * (size_t)im->nder * nwin, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    API_END
}

int smcpp_gamma_cols(smcpp_im *im, int c) {
    if (c < 0 || c >= im->n_contigs) return -1;
    return im->gamma_valid ? im->user_Ls[c] + 1 : 1;
}

int smcpp_get_gamma_argmax(smcpp_im *im, int c, int *out) {
    API_BEGIN
    if (c < 0 || c >= im->n_contigs) throw std::runtime_error("contig index out of range");
    if (!im->gamma_valid) throw std::runtime_error("save_gamma was not set for the last E-step");
    HIPCHK(hipSetDevice(im->device));
    const int L = im->Ls[c];
    im->fetch_stats();
    // (rows cut into pieces: the pieces' posteriors are added up on the device first; L = the caller's row count then)
    const double *src = im->split_spans ? im->merged_gamma(c) : (const double *)(im->d_gamma_rows.p + (size_t)im->contig_base[c] * im->Mp);
    const int Lc = im->split_spans ? im->user_Ls[c] : L;
    im->d_argmax.alloc((size_t)im->total_rows);
    hipLaunchKernelGGL(k_gamma_argmax, dim3(ceil_div(Lc + 1, 256)), dim3(256), 0, im->stream, im->M, im->Mp,
                       (long long)(Lc + 1), src, im->d_argmax.p);
    HIPCHK(hipMemcpyAsync(out, im->d_argmax.p, sizeof(int) * (Lc + 1), hipMemcpyDeviceToHost, im->stream));
    HIPCHK(hipStreamSynchronize(im->stream));
    // column 0 is alpha_0 o beta_0 (hmm.cpp:150), which lives in gamma0
    int best = 0;
    for (int i = 1; i < im->M; ++i)
        if (im->h_gamma0[(size_t)c * im->M + i] > im->h_gamma0[(size_t)c * im->M + best]) best = i;
    out[0] = best;
    API_END
}

int smcpp_get_gamma_sums(smcpp_im *im, int c, double *vals, unsigned char *present) {
    API_BEGIN
    if (c < 0 || c >= im->n_contigs) throw std::runtime_error("contig index out of range");
    im->fetch_stats();
    std::memcpy(vals, &im->h_gsum[(size_t)c * im->K * im->M], sizeof(double) * im->K * im->M);
    std::memcpy(present, &im->present[(size_t)c * im->K], im->K);
    API_END
}

int smcpp_get_pi(smcpp_im *im, double *out) {
    API_BEGIN
    if (im->pi.empty()) throw std::runtime_error("parameters are not set");
    std::memcpy(out, im->pi.data(), sizeof(double) * im->M);
    API_END
}
int smcpp_get_transition(smcpp_im *im, double *out) {
    API_BEGIN
    im->ensure_T();
    if (im->T.empty()) throw std::runtime_error("parameters are not set");
    std::memcpy(out, im->T.data(), sizeof(double) * im->M * im->M);
    API_END
}
int smcpp_get_emission_probs(smcpp_im *im, double *out) {
    API_BEGIN
    im->sync_host_E();
    if (im->E.empty()) throw std::runtime_error("parameters are not set");
    std::memcpy(out, im->E.data(), sizeof(double) * im->K * im->M);
    API_END
}

// ---- derivative-carrying getters (what the binding wraps into ad numbers, _smcpp.pyx:103-120,215-275) ----
static void need_model_params(smcpp_im *im) {
    if (im->have_raw) throw std::runtime_error("parameters were set with set_raw: no model, no derivatives");
    im->prepare_params();
}
int smcpp_get_pi_jac(smcpp_im *im, double *out) {
    API_BEGIN
    need_model_params(im);
    if (im->nder > 0) std::memcpy(out, im->dpi.data(), sizeof(double) * im->dpi.size());
    API_END
}
int smcpp_get_transition_jac(smcpp_im *im, double *out) {
    API_BEGIN
    need_model_params(im);
    im->ensure_dT();
    if (im->nder > 0) std::memcpy(out, im->dT.data(), sizeof(double) * im->dT.size());
    API_END
}
int smcpp_get_emission_probs_jac(smcpp_im *im, double *out) {
    API_BEGIN
    need_model_params(im);
    im->sync_host_E();
    if (im->nder > 0) std::memcpy(out, im->dE.data(), sizeof(double) * im->dE.size());
    API_END
}
int smcpp_num_emission_cols(smcpp_im *im) {
    int cols = 1;
    for (int p = 0; p < im->npop; ++p) cols *= (im->na[p] + 1) * (im->n[p] + 1);
    return cols;
}
int smcpp_get_emission(smcpp_im *im, double *out, double *jac) {
    API_BEGIN
    need_model_params(im);
    im->sync_host_E();
    if (im->emission.size() != (size_t)im->M * smcpp_num_emission_cols(im)) throw std::runtime_error("emission matrix is not available");
    std::memcpy(out, im->emission.data(), sizeof(double) * im->emission.size());
    if (jac && im->nder > 0) std::memcpy(jac, im->demission.data(), sizeof(double) * im->demission.size());
    API_END
}

void smcpp_init_logger_cb(void (*cb)(const char *, const char *, const char *)) { g_logger_cb = cb; }

int smcpp_init_cache(const char *path) {
    API_BEGIN
    smcpp_host::csfs_cache_prefix() = path ? path : "";
    API_END
}

int smcpp_set_global_keys(smcpp_im *im, int Kg, const int *gkeys) {
    API_BEGIN
    const int kl = im->keylen;
    std::map<std::vector<int>, int> gm;
    for (int k = 0; k < Kg; ++k) gm[std::vector<int>(gkeys + (size_t)k * kl, gkeys + (size_t)(k + 1) * kl)] = k;
    im->local_to_global.assign(im->K, -1);
    for (int k = 0; k < im->K; ++k) {
        auto it = gm.find(std::vector<int>(im->keys.begin() + (size_t)k * kl, im->keys.begin() + (size_t)(k + 1) * kl));
        if (it == gm.end()) throw std::runtime_error("global key list misses a local key");
        im->local_to_global[k] = it->second;
    }
    im->gkeys.assign(gkeys, gkeys + (size_t)Kg * kl);
    im->have_global = true;
    im->pack_tables_ready = false;
    if (im->dprep) im->dprep->keys_ready = false;
    if (im->qdev) im->qdev->stats_ready = false;
    im->E_on_dev = false;
    im->params_fresh = false;              // the emission table is now prepared over the global key list
    im->Eg.clear(); im->dEg.clear();
    API_END
}

int smcpp_pack_stats(smcpp_im *im, double *buf, long *n_out, int dev) {
    API_BEGIN
    const int M = im->M, K = im->K;
    const int Kg = im->have_global ? (int)(im->gkeys.size() / im->keylen) : K;
    const long n = 1 + M + (long)M * M + (long)Kg * M;
    if (n_out) *n_out = n;
    if (!buf) return 0;
    if (dev && !im->estep_done) throw std::runtime_error("no E-step has been run on this manager yet");
    if (dev) {
        // device path: one kernel writes the packed layout into the caller's device buffer (e.g. the tensor that is
        // all-reduced over RCCL) - no host round trip
        HIPCHK(hipSetDevice(im->device));
        if (!im->pack_tables_ready) {
            std::vector<int> g2l(Kg, -1);
            for (int k = 0; k < K; ++k) g2l[im->have_global ? im->local_to_global[k] : k] = k;
            im->d_g2l.upload(g2l, im->stream);
            im->d_present.upload(im->present, im->stream);
            HIPCHK(hipStreamSynchronize(im->stream));
            im->pack_tables_ready = true;
        }
        PackArgs pa;
        pa.M = M; pa.Mp = im->Mp; pa.K = K; pa.Kg = Kg; pa.n_contigs = im->n_contigs;
        pa.loglik = im->d_loglik.p; pa.gamma0 = im->d_gamma0.p; pa.xisum = im->d_xisum.p; pa.gsum = im->d_gsum.p;
        pa.present = im->d_present.p; pa.g2l = im->d_g2l.p; pa.out = buf;
        hipLaunchKernelGGL(k_pack_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, im->stream, pa);
        HIPCHK(hipGetLastError());
        // dev == 2: stream-ordered hand-over - the caller consumes `buf` on the engine's stream (smcpp_stream), e.g. an RCCL
        // all-reduce enqueued behind the pack kernel, so there is no host wait between the E-step and the collective
        if (dev != 2) HIPCHK(hipStreamSynchronize(im->stream));
        return 0;
    }
    im->fetch_stats();
    std::vector<double> h(n, 0.0);
    for (int c = 0; c < im->n_contigs; ++c) {
        h[0] += im->loglik[c];
        for (int i = 0; i < M; ++i) h[1 + i] += im->h_gamma0[(size_t)c * M + i];
        for (size_t i = 0; i < (size_t)M * M; ++i) h[1 + M + i] += im->h_xisum[(size_t)c * M * M + i];
        for (int k = 0; k < K; ++k) {
            if (!im->present[(size_t)c * K + k]) continue;
            const int kg = im->have_global ? im->local_to_global[k] : k;
            for (int i = 0; i < M; ++i) h[1 + M + (size_t)M * M + (size_t)kg * M + i] += im->h_gsum[((size_t)c * K + k) * M + i];
        }
    }
    std::memcpy(buf, h.data(), sizeof(double) * n);
    API_END
}

int smcpp_unpack_stats(smcpp_im *im, const double *buf, long n, int dev) {
    API_BEGIN
    const int M = im->M;
    const int Kg = im->have_global ? (int)(im->gkeys.size() / im->keylen) : im->K;
    if (n != 1 + M + (long)M * M + (long)Kg * M) throw std::runtime_error("unpack_stats: wrong buffer length");
    if (!im->have_global) {
        im->local_to_global.resize(im->K);
        for (int k = 0; k < im->K; ++k) im->local_to_global[k] = k;
        im->gkeys = im->keys;
    }
    im->g_stats.resize(n);
    if (dev) {
        HIPCHK(hipSetDevice(im->device));
        HIPCHK(hipMemcpy(im->g_stats.data(), buf, sizeof(double) * n, hipMemcpyDeviceToHost));
    } else std::memcpy(im->g_stats.data(), buf, sizeof(double) * n);
    im->have_reduced = true;
    if (im->qdev) im->qdev->stats_ready = false;
    API_END
}

}  // extern "C"
