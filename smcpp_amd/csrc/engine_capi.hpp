// engine_capi.hpp - part of the ONE translation unit engine.hip (included there, in order; not a standalone header):
// the C ABI of include/smcpp_engine.h - create / destroy, setters, E-step, Q, getters, statistics packing (the products' entry points
// are in engine_products.hpp).
// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
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

int smcpp_set_theta(smcpp_im *im, double v) { API_BEGIN im->theta = v; im->params_changed(true); API_END }
int smcpp_set_rho(smcpp_im *im, double v) { API_BEGIN im->rho = v; im->params_changed(true); API_END }
int smcpp_set_alpha(smcpp_im *im, double v) { API_BEGIN im->alpha = v; im->params_changed(true); API_END }

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
    im->have_model = true;
    im->params_changed(true);
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
    im->have_model = true;
    im->params_changed(true);
    API_END
}

int smcpp_set_prep_mode(smcpp_im *im, int host) {
    API_BEGIN
    im->force_host_prep = host != 0;
    im->params_changed(false);
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
    im->params_on_host_route();
    im->dirty = true;
    im->nder = 0;
    im->param_plan = im->resolve_param_plan();
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
    im->params_changed(true);
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
    im->E_on_dev = false;                  // (the device's table is dropped, not fetched; the rest of the residency state stands)
    im->params_changed(false, false);      // the emission table is now prepared over the global key list
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

// ---- the chain plan: chunking, which family runs, what was planned ---------------------------------------------------------
int smcpp_set_chunking(smcpp_im *im, int rows_per_chunk, double eps_alpha, double eps_beta) {
    API_BEGIN
    HIPCHK(hipSetDevice(im->device));
    if (eps_alpha > 0) im->eps_f = (float)eps_alpha;
    if (eps_beta > 0) im->eps_b = eps_beta;
    if (rows_per_chunk != im->user_rows_per_chunk) {
        im->user_rows_per_chunk = rows_per_chunk;
        im->warm_valid = false;
        im->make_chunks();
        im->upload_chunk_state();
        im->setup_power();
        im->last_fwd_passes = im->last_bwd_passes = 0;
    }
    API_END
}

// which chain kernels this manager runs: 2 cooperative, 3 cooperative with streamed operands,
// 4 lock-step on the matrix cores (chosen at construction / smcpp_set_chunking from the state count and the input size)
// 5 = scans over the semiseparable structure of T (chains_ss.hpp; the dense kernels named by the other values remain the
// fallback of an E-step whose T has no such structure)
// (6 = those with hybrid rows)
static int chain_family(const ChainPlan &p) { return p.scan ? (p.hybrid ? 6 : 5) : (int)p.dense; }
int smcpp_chain_mode(smcpp_im *im) { return im ? chain_family(im->plan) : -1; }

// Test hook (tests/test_gpu_seams.py): the chunk list of one direction as cut_chunks left it, (contig, r0, r1, h0, h1) per chunk.
int smcpp_debug_chunks(smcpp_im *im, int backward, int cap, int *out) {
    if (!im) return -1;
    const std::vector<Chunk> &v = backward ? im->chunks_b : im->chunks;
    for (size_t j = 0; j < v.size() && (long long)j < (long long)cap && out; ++j) {
        const Chunk &ch = v[j];
        const int t[5] = {ch.contig, ch.r0, ch.r1, ch.h0, ch.h1};
        std::copy(t, t + 5, out + 5 * j);
    }
    return (int)v.size();
}

// Every SMCPP_* switch is parsed once per process (engine_options.hpp); this re-reads the environment.
void smcpp_reload_options(void) { smcpp_opt::reload(); }

// The "hybrid" object of smcpp_describe, beside "plan": which form of the hybrid rows' eigen-power step the manager's ChainPlan holds
// (null: no hybrid rows) - the values run_chains_ss hands to SsArgs, nothing recomputed.  Eigen keys by their index (the order of the
// key list among the keys of span > 1 rows); cold: no LDS slot, table rows from L2; hot: the key whose rows stay in registers (Mp = 32).
static std::string describe_hybrid(const smcpp_im *im) {
    static const char *const form[] = {"", "all tables", "direction split", "direction split, cold keys"};
    const ChainPlan &p = im->plan;
    if (!p.hybrid) return ", \"hybrid\": null";
    std::string cold;
    for (int e = 0; e < im->Ke; ++e)
        if (p.eslot_of_key[e] < 0) cold += (cold.empty() ? "" : ", ") + std::to_string(e);
    char t[512];
    snprintf(t, sizeof t, ", \"hybrid\": {\"form\": \"%s\", \"threshold\": %d, \"eigen_keys\": %d, \"tables_in_lds\": %d, \"cold_eigen_keys\": [%s], "
             "\"hot_eigen_key\": %d, \"workgroup_wavefronts\": %d, \"emission_slots_in_lds\": %d, \"all_keys_in_lds\": %s}",
             form[p.hybrid], p.hyb_th, im->Ke, p.nk_lds, cold.c_str(), im->Mp == 32 ? std::max(0, im->hot_eig) : -1, p.wg_waves, p.nlds,
             p.all_keys_in_lds ? "true" : "false");
    return t;
}

// The "plan" object of smcpp_describe (with "power_jumps" inside): every value read from the manager's ChainPlan, the ChainPass of its
// last E-step on the scan chains, or what the E-steps learned; the "hybrid" object follows it.  smcpp_host_chain_plan prints a
// host-only manager through it.
static std::string describe_chain_plan(const smcpp_im *im) {
    char t[1024];
    const ChainPlan &p = im->plan;
    const ChainPass &cp = im->chain_pass;
    std::string s;
    snprintf(t, sizeof t,
             ", \"plan\": {\"chain_family\": %d, \"scan_chains\": %s, \"hybrid_rows\": %s, \"states\": %d, \"states_padded\": %d, "
             "\"states_per_lane\": %d, \"keys\": %d, \"eigen_keys\": %d, \"rows\": %lld, \"positions\": %lld, \"max_span\": %d, "
             "\"chunks_forward\": %zu, \"chunks_backward\": %zu, \"wavefronts_per_simd\": %d, \"halo_pass\": %s, "
             "\"light_passes_forward\": %d, \"light_passes_backward\": %d, \"float_scans_in_stored_passes\": %s, \"two_row_scans\": %s, "
             "\"passes_to_certificate\": %d, \"passes_launched\": %d, \"certificate_pass_launched_up_front\": %s, "
             "\"save_gamma\": %s, \"eigen_free_statistics\": %s, \"per_row_gamma\": \"%s\", \"long_rows_cut\": %s, \"warm_start\": %s, \"host_threads\": %d",
             chain_family(p), p.scan ? "true" : "false", p.hybrid ? "true" : "false", im->M, im->Mp, im->NPL, im->K, im->Ke,
             (long long)(im->total_rows - im->n_contigs), p.positions, im->ss_max_span, im->chunks.size(),
             im->chunks_b.size(), p.wpc, (p.scan && cp.use_halo) ? "true" : "false", cp.light_f, cp.light_b,
             (p.scan && cp.mixed) ? "true" : "false", (p.scan && p.two_row_scans) ? "true" : "false", im->last_ss_passes, im->ss_launched,
             // (the switch and the learned flag as they stand now, not as the last E-step found them)
             im->resolve_chain_pass().cert_up_front ? "true" : "false", im->save_gamma ? "true" : "false",
             im->estep_route.eigfree ? "true" : "false", !im->save_gamma ? "none" : im->estep_route.eigfree ? "scan steps" : im->stats_plan.gamma_form == StatsPlan::GAMMA_PIECES ? "eigen-power pieces + scan steps" : "eigensystem", im->split_spans ? "true" : "false",
             im->warm_start ? "true" : "false", omp_get_max_threads());
    s += t;
    // power jumps of the scan chains: `eligible` is the manager's decision (input, state count, SMCPP_SS_JUMP), `run` whether the
    // last E-step's launches jumped; key = index into the caller's key list, -1 = none
    const bool el = im->ss_jump_on();
    snprintf(t, sizeof t, ", \"power_jumps\": {\"eligible\": %s, \"run\": %s, \"key\": %d, \"key_slot\": %d, \"powers\": [%s]}}",
             el ? "true" : "false", cp.jump ? "true" : "false", el ? p.jump_kid : -1,
             el && !im->ss_slot_of_key.empty() ? im->ss_slot_of_key[p.jump_kid] : -1, el ? std::to_string(p.jump_P).c_str() : "");
    return s + t + describe_hybrid(im);
}

// "parameters" of smcpp_describe: the plan of the last prepare_params() / set_raw, where the tables live NOW, the last E-step's route
static std::string describe_param_plan(const smcpp_im *im) {
    static const char *const source[] = {"", "RAW", "ONEPOP_HOST", "ONEPOP_DEVICE", "TWOPOP_HOST", "TWOPOP_DEVICE_BATCH"};
    static const char *const why[] = {"none", "switch", "prep mode", "size not supported", "literal CSFS", "derivative seeds (two populations)"};
    const ParamPlan &p = im->param_plan;
    const bool seeds = !im->have_raw && im->nder > 0; char t[512];
    snprintf(t, sizeof t, ", \"parameters\": {\"source\": \"%s\", \"why_host\": \"%s\", \"emission_table\": \"%s\", \"transition\": \"%s\", "
             "\"transition_jacobian\": \"%s\", \"key_list\": \"%s\", \"eigen_free_statistics\": %s, \"lean\": %s}", source[p.source], why[p.why_host], im->E_on_dev ? "device" : "host",
             im->T_lazy ? "generators" : "expanded", !seeds ? "none" : im->dT_valid ? "expanded" : "planes", p.global_keys ? "global" : "local",
             im->estep_route.eigfree ? "true" : "false", im->estep_route.eigfree ? "true" : "false");       // (lean = eigen-free statistics on the scan chains)
    return p.source != ParamPlan::NONE ? t : ", \"parameters\": null";
}

// "statistics" of smcpp_describe: the statistics plan of the last E-step (null before the first one) - the stream of every branch, the
// form of every kernel family.  smcpp_host_stats_plan prints a host-only manager through it.
static std::string describe_stats_plan(const smcpp_im *im) {
    char t[1024];
    const StatsPlan &p = im->stats_plan;
    static const char *const stream[] = {"main", "second", "third", "high priority"}, *const rank[] = {"per slab", "teams", "wide"};
    static const char *const eigen[] = {"none", "fold on the scans", "fold on the matrix cores", "generation 2", "classic"};
    static const char *const gsum[] = {"one pass", "own stream", "span > 1 tail", "span-1 branch"};
    static const char *const gamma[] = {"none", "scan steps", "eigen-power pieces + scan steps", "eigensystem batches", "eigensystem rows"};
    snprintf(t, sizeof t,
             ", \"statistics\": {\"span_gt1_stream\": \"%s\", \"span1_stream\": \"%s\", \"gamma_sums_stream\": \"%s\", "
             "\"loglik_stream\": \"%s\", \"per_row_gamma_stream\": \"%s\", \"span1_form\": \"%s\", \"rank_update\": \"%s\", "
             "\"eigen\": \"%s\", \"span_gt1_rank_early\": %s, \"gamma_sums_reduced\": \"%s\", \"per_row_gamma\": \"%s\", "
             "\"per_row_gamma_beside\": %s, \"slab_rows_span1\": %d, \"slab_rows_span_gt1\": %d, \"reduction_shares\": %d}",
             stream[p.span_gt1], stream[p.span1], stream[p.gsum], stream[p.loglik], stream[p.gamma], p.s1_one_pass ? "one pass" : "two kernels",
             rank[p.rank], eigen[p.eigen], p.rank_early ? "true" : "false", gsum[p.gsum_at], gamma[p.gamma_form], p.gamma_beside ? "true" : "false",
             im->lay.slab_rows_1, im->lay.slab_rows_e, im->lay.ZS);
    return p.resolved ? t : ", \"statistics\": null";
}

// One JSON object: the switches found in the environment and the plan this manager resolved from them and from its input (chain
// family, states per lane, chunk counts, history passes, arithmetic of the stored passes and the statistics plan of the LAST
// E-step).  Returns the length the text needs (without the terminating zero); writes at most cap - 1 characters.
int smcpp_describe(smcpp_im *im, char *buf, int cap) {
    std::string s = "{";
    s += smcpp_opt::describe_options();
    if (im) {
        char t[1024];
        s += describe_chain_plan(im);
        s += describe_stats_plan(im);
        // who evaluated the last smcpp_q: the device kernels (q_device), the host loops, or nobody yet
        static const char *const route[] = {"none", "device", "host"};
        s += std::string(", \"q_route\": \"") + route[im->q_route] + "\"";
        s += describe_param_plan(im);
        // the last E-step: did it run twice (the scan chains' attempt on a device-prepared table abandoned for DevPrep flag 2, then the
        // dense kernels) and why; the chain family it ended on (the plan's, or the plan's dense fallback; -1: no E-step yet); why a
        // manager planned for the scan chains fell back ("": it did not)
        s += std::string(", \"estep_redone\": ") + (im->estep_redone ? "1" : "0") + ", \"estep_redone_why\": \"" + im->estep_redone_why + "\"";
        s += ", \"estep_chain_family\": " + std::to_string(!im->estep_done ? -1 : im->estep_route.ss_active ? chain_family(im->plan) : (int)im->plan.dense);
        s += std::string(", \"scan_chains_refused\": \"") + (!im->estep_done || !im->plan.scan || im->estep_route.ss_active ? ""
                 : im->ss_underflow ? "emission underflow" : "transition structure") + "\"";
        // the launch shape of the last posterior path call - paths per wavefront, batches, wavefronts - and the wavefronts of the
        // last posterior transition call (0: none yet); a wavefront takes more than one batch / row where there are fewer of them
        s += ", \"path_batch\": " + std::to_string(im->pp_batch) + ", \"path_batches\": " + std::to_string(im->pp_batches);
        s += ", \"path_waves\": " + std::to_string(im->pp_waves) + ", \"transition_waves\": " + std::to_string(im->pt_waves);
        // ... and of the last posterior position call: its wavefronts and the engine rows it walked
        s += ", \"position_waves\": " + std::to_string(im->pq_waves) + ", \"position_rows_walked\": " + std::to_string(im->pq_walked);
        // ... and of the last simulate call: its wavefronts, its (contig, replicate) pairs and the loud positions it wrote
        s += ", \"simulate_waves\": " + std::to_string(im->sim_waves) + ", \"simulate_units\": " + std::to_string(im->sim_units);
        s += ", \"simulate_events\": " + std::to_string(im->sim_events);
        // ... and of the last log-likelihood track call: the engine rows it walked, its wavefronts and how far the walk of a row
        // from the stored float vector moved the row's evidence at worst, |A_span / log c_r - 1|
        snprintf(t, sizeof t, ", \"ll_items\": %lld, \"ll_waves\": %d, \"ll_walk_worst_ratio\": %.6g", im->ll_nitems, im->ll_waves, im->ll_worst);
        s += t;
        // ... and of the last score track call: the engine rows it walked, its wavefronts and where a block's vectors are parked
        s += ", \"score_items\": " + std::to_string(im->sc_items) + ", \"score_waves\": " + std::to_string(im->sc_waves);
        s += std::string(", \"score_park\": \"") + (im->sc_vectors ? "global" : "lds") + "\", \"score_form\": \"" + (im->sc_vectors ? "vectors" : "matrix") + "\"";
        // ... and of the last exact score windows call: the engine rows a window boundary cut, their segments and the wavefronts of
        // the segment walk (0: no row was cut and it was not launched)
        s += ", \"score_exact_items\": " + std::to_string(im->sx_nitems) + ", \"score_exact_segments\": " + std::to_string(im->sx_nseg);
        s += ", \"score_exact_waves\": " + std::to_string(im->sx_waves);
    }
    s += "}";
    if (buf && cap > 0) {
        const size_t n = std::min(s.size(), (size_t)cap - 1);
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int)s.size();
}

}  // extern "C"
