// engine_plans.hpp - part of the ONE translation unit engine.hip (included there, in order; not a standalone header):
// launch plans: chain families, the scan chains' fixed point, statistics, the E-step.
// ---------------------------------------------------------------------------------------------------------------
// kernel launches
// ---------------------------------------------------------------------------------------------------------------
// Raise a kernel's dynamic LDS limit to 160 KiB, once per kernel (the attribute holds for the process)
template <auto KERNEL>
static void lds_limit_once() {
    static bool once = false;
    if (!once) { HIPCHK(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); once = true; }
}

// the cooperative chains (chains2.hpp): pass 0 and the re-run passes are separate instantiations
template <int MT_, bool TAB_, bool RERUN_, bool HOT2_>
static void launch_chain_coop2_tt(bool fwd, const ChainArgs &a, const CoopArgs &ca, size_t shm, hipStream_t s) {
    if (fwd) {
        lds_limit_once<k_fwd_coop2<MT_, TAB_, RERUN_, HOT2_>>();
        hipLaunchKernelGGL((k_fwd_coop2<MT_, TAB_, RERUN_, HOT2_>), dim3(a.nchunks), dim3(MT_ * 4), shm, s, a, ca);
    } else {
        lds_limit_once<k_bwd_coop2<MT_, TAB_, RERUN_, HOT2_>>();
        hipLaunchKernelGGL((k_bwd_coop2<MT_, TAB_, RERUN_, HOT2_>), dim3(a.nchunks), dim3(MT_ * 4), shm, s, a, ca);
    }
}
template <int MT_, bool TAB_>
static void launch_chain_power_t(bool fwd, const ChainArgs &a, const CoopArgs &ca, size_t shm, hipStream_t s) {
    if (fwd) {
        lds_limit_once<k_fwd_coop2<MT_, TAB_, false, false, true>>();
        hipLaunchKernelGGL((k_fwd_coop2<MT_, TAB_, false, false, true>), dim3(a.nchunks), dim3(MT_ * 4), shm, s, a, ca);
    } else {
        lds_limit_once<k_bwd_coop2<MT_, TAB_, false, false, true>>();
        hipLaunchKernelGGL((k_bwd_coop2<MT_, TAB_, false, false, true>), dim3(a.nchunks), dim3(MT_ * 4), shm, s, a, ca);
    }
}
template <int MT_, bool TAB_, bool RERUN_>
static void launch_chain_coop2_t(bool fwd, const ChainArgs &a, const CoopArgs &ca, size_t shm, hipStream_t s) {
    // without a second eigen key the 64 VGPRs of its operands are not allocated (measured on the whole genome: keeping
    // it beats the extra occupancy, 33.2 vs 36.6 ms - the L2 path of a non-resident key costs more than a lost wavefront)
    if (a.hot2 >= 0) launch_chain_coop2_tt<MT_, TAB_, RERUN_, true>(fwd, a, ca, shm, s);
    else launch_chain_coop2_tt<MT_, TAB_, RERUN_, false>(fwd, a, ca, shm, s);
}
template <int MT_, bool TAB_>
static void launch_chain_coop_t(bool fwd, const ChainArgs &a, const CoopArgs &ca, size_t shm, hipStream_t s) {
    if (a.variant == 1) launch_chain_power_t<MT_, TAB_>(fwd, a, ca, shm, s);
    else if (a.pass > 0 && a.variant != 2) launch_chain_coop2_t<MT_, TAB_, true>(fwd, a, ca, shm, s);
    else launch_chain_coop2_t<MT_, TAB_, false>(fwd, a, ca, shm, s);
}
static bool launch_chain_coop(bool fwd, int Mp, const ChainArgs &a, const CoopArgs &ca, int tab, size_t shm, hipStream_t s) {
    switch (Mp) {
#define C_(x) case x: if (tab) launch_chain_coop_t<x, true>(fwd, a, ca, shm, s); else launch_chain_coop_t<x, false>(fwd, a, ca, shm, s); return true;
        C_(16) C_(32) C_(48) C_(64)
#undef C_
        default: return false;
    }
}

template <int MT_>
static void launch_chain_big_t(bool fwd, const ChainArgs &a, const BigArgs &qa, hipStream_t s) {
    if (a.variant == 1) {          // eigen-free pre-pass
        if (fwd) hipLaunchKernelGGL((k_fwd_big<MT_, true>), dim3(a.nchunks), dim3(MT_ * 4), 0, s, a, qa);
        else hipLaunchKernelGGL((k_bwd_big<MT_, true>), dim3(a.nchunks), dim3(MT_ * 4), 0, s, a, qa);
        return;
    }
    if (fwd) hipLaunchKernelGGL((k_fwd_big<MT_>), dim3(a.nchunks), dim3(MT_ * 4), 0, s, a, qa);
    else hipLaunchKernelGGL((k_bwd_big<MT_>), dim3(a.nchunks), dim3(MT_ * 4), 0, s, a, qa);
}
template <int MT_>
static void launch_chain_lock_t(bool fwd, const ChainArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)((a.nchunks + LOCK_NC - 1) / LOCK_NC)), block(MT_ * 4);
    if (fwd) {
        if (a.pass > 0) hipLaunchKernelGGL((k_fwd_lock<MT_, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_fwd_lock<MT_, false>), grid, block, 0, s, a);
    } else {
        if (a.pass > 0) hipLaunchKernelGGL((k_bwd_lock<MT_, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_bwd_lock<MT_, false>), grid, block, 0, s, a);
    }
}
static bool launch_chain_lock(bool fwd, int Mp, const ChainArgs &a, hipStream_t s) {
    switch (Mp) {
        case 16: launch_chain_lock_t<16>(fwd, a, s); return true;
        case 32: launch_chain_lock_t<32>(fwd, a, s); return true;
        case 48: launch_chain_lock_t<48>(fwd, a, s); return true;
        case 64: launch_chain_lock_t<64>(fwd, a, s); return true;
        default: return false;
    }
}
static bool launch_chain_big(bool fwd, int Mp, const ChainArgs &a, const BigArgs &qa, hipStream_t s) {
    switch (Mp) {
#define B_(x) case x: launch_chain_big_t<x>(fwd, a, qa, s); return true;
        B_(80) B_(96) B_(112) B_(128) B_(144) B_(160) B_(176) B_(192) B_(208) B_(224) B_(240) B_(256)
#undef B_
        default: return false;
    }
}

static void launch_uw(int nt, const UWArgs &a, hipStream_t s) {
    switch (nt) {
#define C_(x) case x: hipLaunchKernelGGL(k_eig_uw<x>, dim3(a.nslabs), dim3(64), 0, s, a); break;
        C_(1) C_(2) C_(3) C_(4) C_(5) C_(6) C_(7) C_(8) C_(9) C_(10) C_(11) C_(12) C_(13) C_(14) C_(15) C_(16)
#undef C_
        default: throw std::runtime_error("unsupported number of hidden states");
    }
}
static void launch_s1(int npl, const S1Args &a, hipStream_t s) {
    switch (npl) {
#define C_(x) case x: hipLaunchKernelGGL(k_s1_scalars<x>, dim3(a.nslabs), dim3(256), 0, s, a); break;
        C_(1) C_(2) C_(3) C_(4) C_(8) C_(16)
#undef C_
        default: throw std::runtime_error("unsupported number of hidden states");
    }
}

ChainArgs smcpp_im::chain_args(const ChainPass &cp) {
    ChainArgs a;
    a.M = M; a.Mp = Mp; a.nchunks = (int)chunks.size(); a.pass = 0;
    a.hot = hot_eig; a.hot2 = hot_eig2; a.variant = 0;
    a.chunks = d_chunks.p; a.rowdesc = d_rowdesc.p + ROWDESC_PAD; a.E = d_E.p; a.dpow = d_dpow.p;
    a.pi_f = d_pi_f.p; a.Tf = d_Tf.p; a.PinvT = d_PinvT.p; a.PT = d_PT.p;
    a.TdT = d_TdT.p; a.Prm = d_Prm.p; a.Pinvrm = d_Pinvrm.p;
    a.alpha = d_alpha.p; a.beta = d_beta.p; a.cnorm = d_cnorm.p;
    a.ends_f = d_ends_f.p; a.used_f = d_used_f.p; a.ends_b = d_ends_b.p; a.used_b = d_used_b.p;
    a.eps_f = eps_f; a.eps_b = eps_b;
    a.dbg = nullptr;
    a.warm_f = nullptr; a.warm_b = nullptr;
    a.Bf = d_Bf.p; a.Bb = d_Bb.p; a.g_span = d_g_span.p; a.nbits = plan.pw_nbits; a.npow = plan.pw_npow;
    a.prio = cp.prio;
    a.changed = nullptr;
    return a;
}

// LDS budget of the cooperative kernels: exchange buffers + descriptors (+ the emission / eigenvalue-power tables when
// they fit: TAB)
static void coop_lds(int Mp, int K, int G, bool tab_allowed, int &tab_c, size_t &shm_c) {
    const int KQ = Mp / 4, UP = KQ + 2;
    const size_t base_c = (size_t)(4 * UP + 8 * UP) * 8 + 2 * Mp * 4 + 1024 + 64;
    const size_t tabs = ((size_t)K * 4 * UP + (size_t)G * Mp) * 8;      // backward layout of generation 1 is the larger one
    tab_c = (base_c + tabs <= 64 * 1024 && tab_allowed) ? 1 : 0;        // (ChainPass::coop_tab = false: the global-table path forced)
    shm_c = base_c + (tab_c ? tabs : 0);
}

// Eigen-free pre-pass: upload pi / T / emission table, build the group powers on the device and launch pass 0 of both
// chains on them; the host then solves the eigenproblems while the GPU runs (estep()).
void smcpp_im::stage_static_and_prepass() {
    ensure_T();
    prepass_launched = false;
    static_packed = false;
    if (!plan.power_ok || (warm_start && warm_valid)) return;
    const ChainPass cp = resolve_chain_pass();
    hipStream_t s = stream, sb = dual_stream ? stream2 : stream;
    const size_t MM = (size_t)Mp * Mp;
    auto ensure = [](auto &v, size_t n, auto init) { if (v.size() != n) v.assign(n, init); };
    ensure(hs_pi_f, (size_t)Mp, 0.f); ensure(hs_Tf, MM, 0.f);
    ensure(hs_TdT, MM, 0.0); ensure(hs_Td, MM, 0.0); ensure(hs_Ep, (size_t)K * Mp, 0.0);
    for (int i = 0; i < M; ++i) {
        hs_pi_f[i] = (float)pi[i];
        for (int j = 0; j < M; ++j) {
            hs_Tf[(size_t)i * Mp + j] = (float)T[(size_t)i * M + j];
            hs_Td[(size_t)i * Mp + j] = T[(size_t)i * M + j];
            hs_TdT[(size_t)j * Mp + i] = T[(size_t)i * M + j];
        }
    }
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < M; ++i) hs_Ep[(size_t)k * Mp + i] = E[(size_t)k * M + i];
    static_packed = true;
    // own small arena (the main one is filled and copied after the eigensolve)
    const size_t need = 8 * 256 + (hs_pi_f.size() + hs_Tf.size()) * 4 + (hs_TdT.size() + hs_Td.size() + hs_Ep.size()) * 8;
    pre_stage.reset(need);
    if (need > pre_cap) {
        if (d_pre) (void)hipFree(d_pre);
        pre_cap = need + need / 4;
        HIPCHK(hipMalloc((void **)&d_pre, pre_cap));
        smcpp_opt::poison(d_pre, pre_cap, __LINE__, __FILE__, true);         // (float / double arrays only)
    }
    size_t off = 0;
    auto put = [&](const void *src, size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        std::memcpy(pre_stage.base + off, src, bytes);
        char *dp = d_pre + off;
        off += bytes;
        return dp;
    };
    ChainArgs a = chain_args(cp);
    if (plan.dense == ChainPlan::STREAMED_OPERANDS) {
        // streamed-operand chains: pi, T (row-major) and the emission table go up, everything else is built on the device
        a.pi_f = reinterpret_cast<const float *>(put(hs_pi_f.data(), hs_pi_f.size() * 4));
        const double *pre_Td = reinterpret_cast<const double *>(put(hs_Td.data(), hs_Td.size() * 8));
        a.E = reinterpret_cast<const double *>(put(hs_Ep.data(), hs_Ep.size() * 8));
        HIPCHK(hipMemcpyAsync(d_pre, pre_stage.base, off, hipMemcpyHostToDevice, s));
        d_changed_f.zero(s);
        d_changed_b.zero(s);
        const int nb = ceil_div((long long)MM, 256);
        hipLaunchKernelGGL(k_big_tq, dim3(nb), dim3(256), 0, s, Mp, pre_Td, d_pre_qTf.p, d_pre_qTdT.p);
        hipLaunchKernelGGL(k_pow_init, dim3(nb, Ke), dim3(256), 0, s, M, Mp, plan.pw_nbits, (const int *)d_e_kid.p, a.E, pre_Td, d_W.p);
        for (int b = 0; b + 1 < plan.pw_nbits; ++b) {
            hipLaunchKernelGGL(k_sq_f64, dim3(Mp / 16, Mp / 16, Ke), dim3(64), 0, s, Mp, (const double *)(d_W.p + (size_t)b * MM),
                               d_W.p + (size_t)(b + 1) * MM, (size_t)plan.pw_nbits * MM);
            if (b + 1 >= 5)
                hipLaunchKernelGGL(k_pow_rescale, dim3(Ke), dim3(256), 0, s, Mp, d_W.p + (size_t)(b + 1) * MM, (size_t)plan.pw_nbits * MM);
        }
        hipLaunchKernelGGL(k_pow_layout, dim3(nb, Ke * plan.pw_nbits), dim3(256), 0, s, Mp, (const double *)d_W.p, d_qBf.p, d_qBb.p);
        pre_bargs = BigArgs();
        pre_bargs.qTf = d_pre_qTf.p; pre_bargs.qTdT = d_pre_qTdT.p;
        pre_bargs.qPinvT = pre_bargs.qPT = pre_bargs.qPrm = pre_bargs.qPinvrm = nullptr;
        pre_bargs.qBf = d_qBf.p; pre_bargs.qBb = d_qBb.p;
        a.variant = 1; a.pass = 0;
        if (sb != s) {
            HIPCHK(hipEventRecord(ev[EV_CHAIN_SYNC], s));
            HIPCHK(hipStreamWaitEvent(sb, ev[EV_CHAIN_SYNC], 0));
        }
        HIPCHK(hipEventRecord(ev[EV_FIRST_PASS], s));
        a.changed = d_changed_f.p;
        launch_chain_big(true, Mp, a, pre_bargs, s);
        HIPCHK(hipEventRecord(ev[EV_PRE_FWD_END], s));
        HIPCHK(hipEventRecord(ev[EV_PRE_BWD_START], sb));
        a.changed = d_changed_b.p;
        launch_chain_big(false, Mp, a, pre_bargs, sb);
        HIPCHK(hipEventRecord(ev[EV_PRE_BWD_END], sb));
        HIPCHK(hipGetLastError());
        prepass_launched = true;
        return;
    }
    a.pi_f = reinterpret_cast<const float *>(put(hs_pi_f.data(), hs_pi_f.size() * 4));
    a.Tf = reinterpret_cast<const float *>(put(hs_Tf.data(), hs_Tf.size() * 4));
    a.TdT = reinterpret_cast<const double *>(put(hs_TdT.data(), hs_TdT.size() * 8));
    const double *pre_Td = reinterpret_cast<const double *>(put(hs_Td.data(), hs_Td.size() * 8));
    a.E = reinterpret_cast<const double *>(put(hs_Ep.data(), hs_Ep.size() * 8));
    HIPCHK(hipMemcpyAsync(d_pre, pre_stage.base, off, hipMemcpyHostToDevice, s));
    d_changed_f.zero(s);
    d_changed_b.zero(s);
    {
        const size_t shm = (size_t)(2 * Mp * (Mp + 1) + 8) * sizeof(double);
        switch (Mp) {
#define P_(x) case x: { static bool once = false; if (!once) { HIPCHK(hipFuncSetAttribute((const void *)k_binary_powers<x>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); once = true; } \
                    hipLaunchKernelGGL(k_binary_powers<x>, dim3(Ke), dim3(256), shm, s, M, plan.pw_npow, (const int *)d_e_kid.p, a.E, pre_Td, d_Bf.p, d_Bb.p); } break;
            P_(16) P_(32) P_(48) P_(64)
#undef P_
            default: throw std::runtime_error("internal: power pre-pass with an unsupported state count");
        }
    }
    const int dbg_level = opt().i(smcpp_opt::O_POWER_DEBUG, 0);
    if (dbg_level == 1) { HIPCHK(hipStreamSynchronize(s)); fprintf(stderr, "[power] powers ok\n"); static_packed = false; return; }
    int tab_c; size_t shm_c;
    coop_lds(Mp, K, G, cp.coop_tab, tab_c, shm_c);
    CoopArgs cargs;
    cargs.K = K; cargs.G = G;
    cargs.power_off = (int)shm_c;          // two scratch vectors behind the regular carve-up
    shm_c += 2048;
    a.variant = 1; a.pass = 0;
    if (!(cp.prio_mask & 1)) a.prio = 0;
    if (sb != s) {
        HIPCHK(hipEventRecord(ev[EV_CHAIN_SYNC], s));
        HIPCHK(hipStreamWaitEvent(sb, ev[EV_CHAIN_SYNC], 0));
    }
    HIPCHK(hipEventRecord(ev[EV_FIRST_PASS], s));
    a.changed = d_changed_f.p;
    launch_chain_coop(true, Mp, a, cargs, tab_c, shm_c, s);
    HIPCHK(hipEventRecord(ev[EV_PRE_FWD_END], s));
    HIPCHK(hipEventRecord(ev[EV_PRE_BWD_START], sb));
    a.changed = d_changed_b.p;
    launch_chain_coop(false, Mp, a, cargs, tab_c, shm_c, sb);
    HIPCHK(hipEventRecord(ev[EV_PRE_BWD_END], sb));
    HIPCHK(hipGetLastError());
    if (dbg_level == 2) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipStreamSynchronize(sb)); fprintf(stderr, "[power] pre-pass ok\n"); }
    prepass_launched = true;
}

void smcpp_im::run_chains() {
    hipStream_t s = stream;
    // what this E-step decides on top of the plan: the passes launched up front, the second stream, the backward chain's issue
    // priority, the warm start (where the buffers of the previous E-step fit this chunk list)
    const ChainPass cp = resolve_chain_pass();
    int want_f = cp.want_f, want_b = cp.want_b;
    const int prio_mask = cp.prio_mask;
    const bool dual = cp.dual;
    const bool warm = cp.warm && d_warm_f.n == chunks.size() * (size_t)Mp && d_warm_b.n == chunks.size() * (size_t)Mp;
    ChainArgs a = chain_args(cp);
    CoopArgs cargs;
    cargs.K = K; cargs.G = G; cargs.power_off = 0;
    BigArgs bargs;
    bargs.qTf = d_qTf.p; bargs.qPinvT = d_qPinvT.p; bargs.qPT = d_qPT.p; bargs.qTdT = d_qTdT.p;
    bargs.qPrm = d_qPrm.p; bargs.qPinvrm = d_qPinvrm.p; bargs.qBf = nullptr; bargs.qBb = nullptr;
    size_t shm_c = 0;
    int tab_c = 0;
    coop_lds(Mp, K, G, cp.coop_tab, tab_c, shm_c);
    a.warm_f = warm ? d_warm_f.p : nullptr;
    a.warm_b = warm ? d_warm_b.p : nullptr;
    if (opt().has(smcpp_opt::O_DEBUG_CYCLES)) { d_dbg.alloc(16); d_dbg.zero(s); a.dbg = d_dbg.p; }
    const bool pre = prepass_launched;      // pass 0 of both chains already runs (eigen-free pre-pass, flags zeroed there)
    if (!pre) {
        d_changed_f.zero(s);
        d_changed_b.zero(s);
    }
    if (h_flags_cap < 2 * (plan.max_pass + 1)) {
        if (h_flags) (void)hipHostFree(h_flags);
        h_flags_cap = 2 * (plan.max_pass + 1);
        HIPCHK(hipHostMalloc((void **)&h_flags, sizeof(int) * h_flags_cap, hipHostMallocCoherent | hipHostMallocMapped));
        d_flags_view = nullptr;
    }
    int *chf = h_flags, *chb = h_flags + (plan.max_pass + 1);
    auto first_quiet = [](const int *ch, int upto) {
        for (int j = 0; j < upto; ++j)
            if (ch[j] == 0) return j;
        return -1;
    };
    int launched_f = pre ? 1 : 0, launched_b = pre ? 1 : 0;
    // after a pre-pass, pass 1 is a FULL pass from the pre-pass's end vectors (no skip test, no merge exit): every stored
    // row then comes from the exact kernels
    // issue priority of the backward wavefronts per pass (SMCPP_BWD_PRIO_MASK: bit 0 pre-pass, bit 1 the full pass after
    // it, bit 2 every other pass)
    const int prio0 = a.prio;
    auto set_variant = [&](int pass) {
        a.pass = pass;
        if (pre && pass == 1) { a.variant = 2; a.warm_f = d_ends_f.p; a.warm_b = d_ends_b.p; a.prio = (prio_mask & 2) ? prio0 : 0; }
        else { a.variant = 0; a.warm_f = warm ? d_warm_f.p : nullptr; a.warm_b = warm ? d_warm_b.p : nullptr; a.prio = (prio_mask & 4) ? prio0 : 0; }
    };
    // The two chains are independent (beta does not depend on alpha).  The cooperative kernels leave most of a CU's
    // LDS and issue slots idle, so the backward passes run on a second stream and share the CUs with the forward ones.
    hipStream_t sb = dual ? stream2 : s;
    // one pass of one chain on the family's kernels
    auto launch_pass = [&](bool fwd, hipStream_t st) {
        if (!(plan.dense == ChainPlan::LOCK_STEP && launch_chain_lock(fwd, Mp, a, st)) &&
            !(plan.dense == ChainPlan::STREAMED_OPERANDS && launch_chain_big(fwd, Mp, a, bargs, st)) &&
            !(plan.dense == ChainPlan::COOPERATIVE && launch_chain_coop(fwd, Mp, a, cargs, tab_c, shm_c, st)))
            throw std::runtime_error("internal: no dense chain kernel for this number of hidden states");
    };
    if (dual) {
        HIPCHK(hipEventRecord(ev[EV_CHAIN_SYNC], s));              // parameters / zeroed flags are ready on the main stream
        HIPCHK(hipStreamWaitEvent(sb, ev[EV_CHAIN_SYNC], 0));
    }
    HIPCHK(hipEventRecord(ev[EV_CHAINS_START], s));
    bool fdone = false, bdone = false;
    int fq = -1, bq = -1;
    bool first_round = true;
    while (true) {
        if (!fdone) {
            a.changed = d_changed_f.p;
            for (; launched_f < want_f; ++launched_f) {
                set_variant(launched_f);
                launch_pass(true, s);
            }
        }
        if (first_round) HIPCHK(hipEventRecord(ev[EV_BWD_START], dual ? sb : s));
        if (!bdone) {
            a.changed = d_changed_b.p;
            for (; launched_b < want_b; ++launched_b) {
                set_variant(launched_b);
                launch_pass(false, sb);
            }
        }
        HIPCHK(hipGetLastError());
        if (first_round && dual) HIPCHK(hipEventRecord(ev[EV_FWD_END], s));      // end of the first batch of forward passes
        HIPCHK(hipMemcpyAsync(chf, d_changed_f.p, sizeof(int) * (plan.max_pass + 1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(chb, d_changed_b.p, sizeof(int) * (plan.max_pass + 1), hipMemcpyDeviceToHost, sb));
        if (dual) {
            HIPCHK(hipEventRecord(ev[EV_CHAIN_SYNC], sb));
            HIPCHK(hipStreamWaitEvent(s, ev[EV_CHAIN_SYNC], 0));   // the statistics (main stream) need both chains
        }
        HIPCHK(hipEventRecord(ev[EV_CHAINS_END], s));
        // Optimistic: the first batch normally contains the quiet pass (it is sized from the previous E-step), so the
        // statistics are queued behind it BEFORE the host waits for the flags - the read-back round trip and their launch
        // latency disappear behind GPU work.  If the flags say otherwise the statistics are simply queued again later.
        if (first_round && !save_gamma) enqueue_stats();
        else stats_enqueued = false;
        HIPCHK(hipStreamSynchronize(s));
        if (dual) HIPCHK(hipStreamSynchronize(sb));
        first_round = false;
        fq = first_quiet(chf, launched_f);
        bq = first_quiet(chb, launched_b);
        fdone = fq >= 0 || launched_f >= plan.max_pass;
        bdone = bq >= 0 || launched_b >= plan.max_pass;
        if (fdone && bdone) break;
        stats_enqueued = false;             // more passes follow: whatever was queued is stale
        if (!fdone) want_f = std::min(plan.max_pass, launched_f + 4);
        if (!bdone) want_b = std::min(plan.max_pass, launched_b + 4);
    }
    chains_dual = dual;
    if (a.dbg) {
        long long h[16];
        HIPCHK(hipMemcpy(h, d_dbg.p, sizeof(h), hipMemcpyDeviceToHost));
        for (int w = 0; w < 4; ++w)
            fprintf(stderr, "[cycles] fwd wg1 wave%d: loop %lld, end-barrier %lld, mid-barrier %lld, rows %lld\n", w, h[4 * w], h[4 * w + 1], h[4 * w + 2], h[4 * w + 3]);
    }
    if (fq < 0 || bq < 0) { stats_enqueued = false; throw std::runtime_error("chunk-boundary iteration did not converge"); }
    last_fwd_passes = fq;
    last_bwd_passes = bq;
    if (warm_start && plan.dense == ChainPlan::COOPERATIVE && Mp <= 64) {
        // every pass after the first quiet one only copies the boundary vectors forward: the buffer of the last
        // launched pass holds the converged ones
        const size_t nel = chunks.size() * (size_t)Mp;
        d_warm_f.alloc(nel); d_warm_b.alloc(nel);
        HIPCHK(hipMemcpyAsync(d_warm_f.p, d_ends_f.p + (size_t)((launched_f - 1) & 1) * nel, nel * sizeof(float),
                              hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(d_warm_b.p, d_ends_b.p + (size_t)((launched_b - 1) & 1) * nel, nel * sizeof(double),
                              hipMemcpyDeviceToDevice, s));
        warm_valid = true;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// chains on the semiseparable structure of T (chains_ss.hpp)
// ---------------------------------------------------------------------------------------------------------------
// The generator arrays lie side by side, gen = [10][MS] in the order f_dc f_g f_cg f_b f_a f_d b_dc b_g b_b b_a, the backward ones
// mirrored (state j at MS - 1 - j): written on the host by ss_pack_generators, handed to a kernel by set_generators.
static void ss_pack_generators(int M, int MS, double c0, const std::vector<double> &d, const std::vector<double> &g,
                               const std::vector<double> &a, const std::vector<double> &b, std::vector<double> &gen) {
    gen.assign((size_t)10 * MS, 0.0);
    double *f = &gen[0], *bw = f + (size_t)6 * MS;
    for (int j = 0; j < M; ++j) {
        f[j] = d[j] - c0; f[MS + j] = g[j]; f[2 * MS + j] = c0 - g[j]; f[3 * MS + j] = b[j]; f[4 * MS + j] = a[j]; f[5 * MS + j] = d[j];
        const int p = MS - 1 - j;
        bw[p] = d[j] - c0; bw[MS + p] = g[j]; bw[2 * MS + p] = b[j]; bw[3 * MS + p] = a[j];
    }
}
// Points the ten generator arrays of `a` at gd (gen on the device) and sets c0.
static void set_generators(SsArgs &a, const double *gd, int MS, double c0) {
    a.f_dc = gd; a.f_g = gd + MS; a.f_cg = gd + 2 * MS; a.f_b = gd + 3 * MS; a.f_a = gd + 4 * MS; a.f_d = gd + 5 * MS;
    a.b_dc = gd + 6 * MS; a.b_g = gd + 7 * MS; a.b_b = gd + 8 * MS; a.b_a = gd + 9 * MS;
    a.c0 = c0;
}

// Generators of T = diag(d) + [below: g_j] + [above: c0 + Phi'(i,j)], Phi'(i,i+1) = b_i, Phi'(i,j+1) = a_j Phi'(i,j)
// (transition.cpp:176-254; c0 = 1e-5 / (M + 1) is the mixing constant of lines 249-254).  The dense T is what the reference's
// getters hand out and what the statistics use, so the generators are taken FROM it and the reconstruction is checked entry by
// entry: a T without this structure (smcpp_set_raw with an arbitrary matrix) sends the E-step to the dense kernels.
static bool ss_generators(int M, int MS, const double *Tm, std::vector<double> &gen, double &c0_out) {
    const double c0 = 1e-5 / (double)(M + 1);
    const double tol = 1e-11;
    std::vector<double> d(M), g(M, 0.0), a(M, 0.0), b(M, 0.0);
    for (int j = 0; j < M; ++j) d[j] = Tm[(size_t)j * M + j];
    for (int j = 0; j + 1 < M; ++j) {
        g[j] = Tm[(size_t)(M - 1) * M + j];
        b[j] = Tm[(size_t)j * M + j + 1] - c0;
    }
    // (both sweeps below walk T row by row: at M = 256 the matrix is 512 KB and a column walk misses the cache on every entry)
    for (int i = 1; i < M; ++i) {
        const double *row = Tm + (size_t)i * M;
        for (int j = 0; j < i && j + 1 < M; ++j)
            if (!(std::fabs(row[j] - g[j]) <= tol * std::fabs(g[j]))) return false;
    }
    {
        // a_j from the row with the LARGEST entry in column j above the diagonal (best conditioned quotient)
        std::vector<int> ib(M, 0);
        std::vector<double> best(M, -1.0);
        for (int i = 0; i + 2 < M; ++i) {
            const double *row = Tm + (size_t)i * M;
            for (int j = std::max(1, i + 1); j + 1 < M; ++j)
                if (row[j] > best[j]) { best[j] = row[j]; ib[j] = i; }
        }
        for (int j = 1; j + 1 < M; ++j) {
            const double den = Tm[(size_t)ib[j] * M + j] - c0;
            a[j] = den > 0.0 ? (Tm[(size_t)ib[j] * M + j + 1] - c0) / den : 0.0;
        }
    }
    for (int i = 0; i + 1 < M; ++i) {
        double v = b[i];
        for (int j = i + 1; j < M; ++j) {
            const double t = Tm[(size_t)i * M + j];
            if (!(std::fabs(c0 + v - t) <= tol * std::fabs(t)) || !(t > 0.0)) return false;
            v *= a[j];
        }
    }
    for (int j = 0; j < M; ++j)
        if (!(d[j] > 0.0) || !std::isfinite(a[j]) || !std::isfinite(b[j])) return false;
    c0_out = c0;
    ss_pack_generators(M, MS, c0, d, g, a, b, gen);
    return true;
}

// The same generators straight from the O(M) quantities the device-prepared model path computed (prep.hpp: TransitionGenJac - below
// the diagonal T(i, c) = ed[c], above it pf[i] W[c], the diagonal closes the row; transition_expand then floors at 1e-20 and mixes with
// c0 = 1e-5 / (M + 1)): no M x M matrix is formed or checked.  The diagonal's row sum is taken from a prefix sum of ed and a suffix sum
// of W instead of entry by entry: 1e-16 of what the expanded matrix holds.
static bool ss_generators_from_tgen(int M, int MS, const smcpp_host::TransitionGenJac &tj, std::vector<double> &gen, double &c0_out) {
    if (!tj.ok || tj.M != M || (int)tj.ed.size() != std::max(0, M - 1) || (int)tj.pf.size() != M || (int)tj.W.size() != M) return false;
    const double beta = 1e-5, c0 = beta / (double)(M + 1), om = 1.0 - beta;
    auto mix = [&](double raw) { return std::max(raw, 1e-20) * om; };          // (without the + c0)
    std::vector<double> d(M), g(M, 0.0), a(M, 0.0), b(M, 0.0), below(M, 0.0), above(M + 1, 0.0);
    for (int j = 1; j < M; ++j) below[j] = below[j - 1] + tj.ed[j - 1];
    for (int c = M - 1; c >= 1; --c) above[c] = above[c + 1] + tj.W[c];            // above[c] = sum_{k >= c} W[k]
    for (int j = 0; j + 1 < M; ++j) {
        g[j] = mix(tj.ed[j]) + c0;
        b[j] = mix(tj.pf[j] * tj.W[j + 1]);
    }
    for (int j = 1; j + 1 < M; ++j) a[j] = tj.W[j] > 0.0 ? tj.W[j + 1] / tj.W[j] : 0.0;
    for (int j = 0; j < M; ++j) d[j] = mix(1.0 - (below[j] + tj.pf[j] * above[j + 1])) + c0;
    for (int j = 0; j < M; ++j)
        if (!(d[j] > 0.0) || !std::isfinite(a[j]) || !std::isfinite(b[j]) || !(b[j] >= 0.0) || (j + 1 < M && !(g[j] > 0.0))) return false;
    c0_out = c0;
    ss_pack_generators(M, MS, c0, d, g, a, b, gen);
    return true;
}

bool smcpp_im::ss_generators_only() {
    if ((T_lazy || T_from_gen) && tgen_valid && ss_generators_from_tgen(M, 64 * NPL, tgen, ss_gen, ss_c0)) {
        // (no expanded matrix yet, and none needed by the chains)
    } else {
        ensure_T();
        if (!ss_generators(M, 64 * NPL, T.data(), ss_gen, ss_c0)) return false;
    }
    return true;
}

bool smcpp_im::ss_extract_generators() {
    ss_underflow = false;
    if (!ss_generators_only()) return false;
    if (ss_range_refused) { ss_underflow = true; return false; }
    // a row of span s applies its operator s times without rescaling: keep clear of underflow
    // (a device-prepared table is checked by the kernel that forms it: DevPrep flag 2, looked at when the chains have drained)
    if (!E_on_dev) for (const Group &gr : groups) {
        if (plan.hybrid && gr.span > plan.hyb_th) continue;          // an eigen-power step, not `span` scan steps
        double mn = 1.0, mx = 0.0;
        for (int i = 0; i < M; ++i) { mn = std::min(mn, E[(size_t)gr.kid * M + i]); mx = std::max(mx, E[(size_t)gr.kid * M + i]); }
        // (prep_dev.hpp has the two bounds and where they come from)
        if (!(mn > 0.0) || (double)gr.span * std::log(mn) < smcpp_dev::SS_SPAN_LOG_MIN ||
            (gr.span > 1 && (double)gr.span * std::log(mx) < smcpp_dev::SS_SPAN_LOG_MAX)) { ss_underflow = true; return false; }
    }
    return true;
}

template <int NPL_, bool HYB_, bool ALL_, bool H32_ = false>
static void launch_chain_ss_tt(const SsArgs &a, int ntasks, size_t shm, hipStream_t s, int wgw) {
    lds_limit_once<k_chain_ss<NPL_, HYB_, ALL_, H32_>>();
    hipLaunchKernelGGL((k_chain_ss<NPL_, HYB_, ALL_, H32_>), dim3(ntasks / wgw), dim3(64 * wgw), shm, s, a);
}
// The instantiation the plan names (ChainPlan::all_keys_in_lds, two_row_scans; describe() reports the latter)
template <int NPL_, bool HYB_>
static void launch_chain_ss_t(const ChainPlan &p, const SsArgs &a, int ntasks, size_t shm, hipStream_t s) {
    if (p.two_row_scans) launch_chain_ss_tt<NPL_, HYB_, true, NPL_ == 1 && !HYB_>(a, ntasks, shm, s, p.wg_waves);
    else if (p.all_keys_in_lds) launch_chain_ss_tt<NPL_, HYB_, true>(a, ntasks, shm, s, p.wg_waves);
    else launch_chain_ss_tt<NPL_, HYB_, false>(a, ntasks, shm, s, p.wg_waves);
}
static void launch_chain_ss(const ChainPlan &p, int npl, const SsArgs &a, int ntasks, size_t shm, hipStream_t s) {
    switch (npl) {
        case 1: if (p.hybrid) launch_chain_ss_t<1, true>(p, a, ntasks, shm, s); else launch_chain_ss_t<1, false>(p, a, ntasks, shm, s); break;
        case 2: launch_chain_ss_t<2, false>(p, a, ntasks, shm, s); break;
        case 3: launch_chain_ss_t<3, false>(p, a, ntasks, shm, s); break;
        case 4: launch_chain_ss_t<4, false>(p, a, ntasks, shm, s); break;
        case 8: launch_chain_ss_t<8, false>(p, a, ntasks, shm, s); break;
        case 16: launch_chain_ss_t<16, false>(p, a, ntasks, shm, s); break;
        default: throw std::runtime_error("unsupported number of hidden states");
    }
}


void smcpp_im::ss_launch_passes(int upto) {
    const size_t shm = (size_t)plan.nlds * 64 * NPL * sizeof(double) + ss_tab_bytes(plan, Mp);
    for (; ss_launched < upto; ++ss_launched) {
        // per direction: `light` store-free float passes (history), then one full pass from their end vectors, then re-run
        // passes; without light passes the first pass is the full one (from pi / the uniform vector)
        const int p = ss_launched;
        const bool lf = p < chain_pass.light_f, lb = p < chain_pass.light_b;
        ss_args.pass = p;
        ss_args.mode_f = lf ? 2 : p == 0 ? 0 : 1;
        ss_args.mode_b = lb ? 2 : p == 0 ? 0 : 1;
        ss_args.full_f = (p > 0 && p == chain_pass.light_f) ? 1 : 0;
        ss_args.full_b = (p > 0 && p == chain_pass.light_b) ? 1 : 0;
        launch_chain_ss(plan, NPL, ss_args, (int)ss_tasks.size(), shm, stream);
    }
    HIPCHK(hipGetLastError());
}

// What this E-step decides on top of the plan; with resolve_chain_plan the only reader of the chain phase's switches.
ChainPass smcpp_im::resolve_chain_pass() const {
    ChainPass cp;
    const bool several = chunks.size() > (size_t)n_contigs && chunks_b.size() > (size_t)n_contigs;   // chunks per contig, both directions
    const bool warm = warm_start && ss_warm_valid;
    // All scans of the stored passes in float (chains_ss.hpp: ss_x_scan_fwd / ss_x_scan_bwd), the default since round 5 for one
    // state per lane; SMCPP_SS_MIXED=0 keeps the fp64 scans (tests and bench.py's `value_ref_width` compare the two).
    // Round 6: with save_gamma as well - the decoded index of EVERY column of the two full-size binned contigs (471 106 columns,
    // goldens G19) equals the compiled reference's under the float scans (tests/test_gpu_argmax.py), so the path that is timed and
    // the path whose indices are checked are the same arithmetic.
    cp.mixed = !opt().off(smcpp_opt::O_SS_MIXED) && NPL == 1 && !plan.hybrid;
    {
        // light passes: enough of them that the full pass starts ~11 e-folds of history in (the chains forget with an e-fold of
        // ~240 positions forward, ~340 backward on the benchmark model); none when the chunks are long against that
        const int ef = opt().i(smcpp_opt::O_SS_LIGHT_F, -1), eb = opt().i(smcpp_opt::O_SS_LIGHT_B, -1);
        const long long pos = plan.positions / std::max<size_t>(1, chunks.size());
        const long long pos_b = plan.positions / std::max<size_t>(1, chunks_b.size());
        auto pick = [&](double hist, long long p_) { return p_ <= 0 || (double)p_ > 1.5 * hist ? 0 : std::min(4, (int)std::ceil(hist / (double)p_)); };
        cp.light_f = ef >= 0 ? ef : pick(2800.0, pos);
        cp.light_b = eb >= 0 ? eb : pick(3900.0, pos_b);
        if (chunks.size() <= (size_t)n_contigs) cp.light_f = 0;      // one chunk per contig: nothing to iterate
        if (chunks_b.size() <= (size_t)n_contigs) cp.light_b = 0;
    }
    if (plan.hybrid) cp.light_f = cp.light_b = 0;      // (the light passes have no eigen-power step; un-binned inputs have long chunks)
    // halo pass: the first pass enters every chunk through its halo and stores rows that are already exact; no light passes
    cp.use_halo = plan.halo && !warm && several;
    if (cp.use_halo) cp.light_f = cp.light_b = 0;
    if (warm && several) {
        // the boundary vectors of the previous E-step are exact for ITS parameters, i.e. off by the parameter step instead of by
        // O(1): they replace one light pass; every stored row still comes from the full fp64 pass on the new parameters
        cp.pass0 = ss_warm_parity == 0 ? 1 : 2;
        cp.light_f = cp.pass0 + std::max(0, cp.light_f - 1);
        cp.light_b = cp.pass0 + std::max(0, cp.light_b - 1);
    }
    cp.jump = ss_jump_on();
    // (round 5) the passes launched up front end with the pass that is expected to rewrite no end vector - the all-skip pass behind
    // it (0.01 ms of kernel + its place in the queue) is not launched: run_chains_ss certifies from the end-vector flags
    cp.cert_up_front = opt().on(smcpp_opt::O_SS_CERT_PASS) || ss_need_cert_pass;
    // (never fewer than one re-run pass behind the pass that stores everything - that one always rewrites its end vectors: with one
    // chunk per contig, or boundaries that were already exact, the quiet pass IS that re-run pass)
    cp.want = std::min(plan.max_pass, std::max(cp.pass0 + (last_ss_passes > 0 ? last_ss_passes + (cp.cert_up_front ? 1 : 0) : 6),
                                               std::max(cp.light_f, cp.light_b) + 2));
    // the dense families: passes launched up front (sized from the previous E-step), the backward chain on a second stream, its
    // issue priority (SMCPP_BWD_PRIO: s_setprio 0..3) and the passes that raise it, the warm start, the LDS tables (test hook)
    cp.want_f = std::min(plan.max_pass, last_fwd_passes > 0 ? last_fwd_passes + 1 : std::min(plan.max_pass, 8));
    cp.want_b = std::min(plan.max_pass, last_bwd_passes > 0 ? last_bwd_passes + 1 : std::min(plan.max_pass, 8));
    cp.dual = dual_stream && ((plan.dense == ChainPlan::COOPERATIVE && Mp <= 64) || plan.dense == ChainPlan::LOCK_STEP || Mp > 64);
    cp.prio = std::max(0, std::min(3, opt().i(smcpp_opt::O_BWD_PRIO, 1)));
    cp.prio_mask = opt().i(smcpp_opt::O_BWD_PRIO_MASK, 7);
    cp.warm = warm_start && warm_valid && plan.dense == ChainPlan::COOPERATIVE && Mp <= 64;
    cp.coop_tab = !opt().has(smcpp_opt::O_COOP_TAB) || opt().i(smcpp_opt::O_COOP_TAB, 1) != 0;
    return cp;
}

// Upload pi, the generators and the emission vectors (by key slot) and start the passes: nothing here needs an eigensystem,
// so the host solves the eigenproblems of the statistics while the chains run.
void smcpp_im::ss_launch_initial() {
    hipStream_t s = stream;
    const ChainPass &cp = chain_pass = resolve_chain_pass();
    const int MS = 64 * NPL;
    std::vector<float> &pi_f = hs_pi_f;
    if (pi_f.size() != (size_t)Mp) pi_f.assign(Mp, 0.f);
    for (int i = 0; i < M; ++i) pi_f[i] = (float)pi[i];
    const size_t need = 12 * 256 + pi_f.size() * 4 + ss_gen.size() * 8 + (size_t)K * MS * 8;
    pre_stage.reset(need);
    if (need > pre_cap) {
        if (d_pre) (void)hipFree(d_pre);
        pre_cap = need + need / 4;
        HIPCHK(hipMalloc((void **)&d_pre, pre_cap));
        smcpp_opt::poison(d_pre, pre_cap, __LINE__, __FILE__, true);         // (float / double arrays only)
    }
    size_t off = 0;
    auto put = [&](const void *src, size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        if (src) std::memcpy(pre_stage.base + off, src, bytes);
        char *dp = d_pre + off;
        off += bytes;
        return dp;
    };
    SsArgs &a = ss_args;
    a = SsArgs();
    a.M = M; a.Mp = Mp; a.nchunks = (int)chunks.size(); a.pass = 0; a.K = K; a.nlds = plan.nlds;
    a.chunks = d_chunks.p; a.rowdesc = d_rowdesc_ss.p + ROWDESC_PAD;
    a.chunks_b = d_chunks_b.p; a.nchunks_b = (int)chunks_b.size(); a.tasks = d_tasks.p;
    a.pi_f = reinterpret_cast<const float *>(put(pi_f.data(), pi_f.size() * 4));
    set_generators(a, reinterpret_cast<const double *>(put(ss_gen.data(), ss_gen.size() * 8)), MS, ss_c0);
    if (E_on_dev) a.E = dprep->d_Es.p;       // written by the device preparation, by key slot
    else {
        const size_t eoff = (off + 255) & ~(size_t)255;
        double *he = reinterpret_cast<double *>(pre_stage.base + eoff);
        std::memset(he, 0, (size_t)K * MS * 8);
        for (int k = 0; k < K; ++k)
            std::memcpy(he + (size_t)ss_slot_of_key[k] * MS, &E[(size_t)k * M], sizeof(double) * M);
        a.E = reinterpret_cast<const double *>(put(nullptr, (size_t)K * MS * 8));
    }
    a.alpha = d_alpha.p; a.beta = d_beta.p; a.cnorm = d_cnorm.p;
    a.ends_f = d_ends_f.p; a.used_f = d_used_f.p; a.ends_b = d_ends_b.p; a.used_b = d_used_b.p;
    {
        // the per-pass flags live in pinned host memory: written by the kernels through its device view, cleared and read by the host
        // ([0, plan.max_pass]: "a chunk of the forward chain re-ran", then the same of the backward chain, then the two "an end vector
        // was rewritten" arrays of the scan chains)
        if (h_flags_cap < 4 * (plan.max_pass + 1)) {
            if (h_flags) (void)hipHostFree(h_flags);
            h_flags_cap = 4 * (plan.max_pass + 1);
            HIPCHK(hipHostMalloc((void **)&h_flags, sizeof(int) * h_flags_cap, hipHostMallocCoherent | hipHostMallocMapped));
            d_flags_view = nullptr;
        }
        if (!d_flags_view) HIPCHK(hipHostGetDevicePointer((void **)&d_flags_view, h_flags, 0));
        if (!h_done) {
            HIPCHK(hipHostMalloc((void **)&h_done, 64, hipHostMallocCoherent | hipHostMallocMapped));
            *h_done = 0;
            HIPCHK(hipHostGetDevicePointer((void **)&d_done_view, h_done, 0));
        }
        std::memset(h_flags, 0, sizeof(int) * h_flags_cap);
    }
    a.changed_f = d_flags_view; a.changed_b = d_flags_view + (plan.max_pass + 1);
    a.endchg_f = d_flags_view + 2 * (plan.max_pass + 1); a.endchg_b = d_flags_view + 3 * (plan.max_pass + 1);
    a.eps_f = eps_f; a.eps_b = eps_b; a.full_f = a.full_b = 0;
    a.mixed = cp.mixed ? 1 : 0;
    if (plan.hybrid) {
        a.hyb_th = plan.hyb_th; a.Ke = Ke; a.hot_ek = std::max(0, hot_eig); a.dirsplit = plan.dirsplit() ? 1 : 0;
        a.nk_lds = plan.nk_lds;
        for (int e = 0; e < 4; ++e) { a.key_of_slot[e] = plan.ekey_of_slot[e]; a.slot_of_key[e] = plan.eslot_of_key[e]; }
        a.Pinvrm = d_Pinvrm.p; a.Prm = d_Prm.p; a.PinvT = d_PinvT.p; a.PT = d_PT.p; a.dsc = d_dsc.p;
    }
    a.halo = cp.use_halo ? 1 : 0;
    ss_warm_valid = false;                     // (set again when this E-step's chains have converged)
    a.dbg = nullptr;
    if (opt().has(smcpp_opt::O_DEBUG_CYCLES)) { d_dbg.alloc(16); d_dbg.zero(s); a.dbg = d_dbg.p; }
    HIPCHK(hipMemcpyAsync(d_pre, pre_stage.base, off, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ev[EV_FIRST_PASS], s));
    {
        // Power jumps: the table of this E-step's operator power is built here, behind the upload above and the device-prepared
        // emission table, in front of the first pass - 64 wavefronts x P dependent scan steps (k_ss_jump_tables)
        a.jump = 0;
        if (cp.jump) {
            d_jtab_f.alloc(2 * 64 * 64);
            d_jdiag.alloc(64);
            a.jump = plan.jump_P; a.jtab_f = d_jtab_f.p; a.jtab_t = d_jtab_f.p + 64 * 64; a.jdiag = d_jdiag.p;
            hipLaunchKernelGGL(k_ss_jump_tables, dim3(16), dim3(256), 0, s, a, ss_slot_of_key[plan.jump_kid], d_jtab_f.p, d_jtab_f.p + 64 * 64, d_jdiag.p);
        }
    }
    ss_launched = cp.pass0;
    ss_launch_passes(cp.want);
    // (no event behind the passes here: run_chains_ss records EV_CHAINS_END at this very position, and every record costs the queue
    // ~3 us in front of the statistics' critical branch - tools/sync_lab.hip)
}

bool smcpp_im::wait_done(int epoch) {
    // poll the pinned word the last kernel of the queue writes; a generous deadline, then the ordinary blocking wait
    const auto t0 = std::chrono::steady_clock::now();
    unsigned n = 0;
    while (__atomic_load_n(h_done, __ATOMIC_ACQUIRE) != epoch) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
        if ((++n & 0x3fff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 5.0) {
            HIPCHK(hipStreamSynchronize(stream));
            return __atomic_load_n(h_done, __ATOMIC_ACQUIRE) == epoch;
        }
    }
    return true;
}

// false: no pass was quiet AND the device preparation flagged its emission table (DevPrep flag 2: the vectors of a long row may have
// underflowed to zero, then 0 x inf) - the caller redoes the E-step on the dense kernels; without the flag that is an error.
bool smcpp_im::run_chains_ss() {
    hipStream_t s = stream;
    const int *chf = h_flags, *chb = h_flags + (plan.max_pass + 1);
    const int p0 = chain_pass.pass0;
    auto first_quiet = [p0](const int *cf, const int *cb, int upto) {
        for (int j = p0; j < upto; ++j)
            if (cf[j] == 0 && cb[j] == 0) return j;
        return -1;
    };
    ss_warm_valid = false;
    bool first_round = true;
    int q = -1, first_launched = -1;      // (first_launched: passes launched when the first round failed to certify, -1: it did)
    const bool poll = !opt().off(smcpp_opt::O_POLL);
    while (true) {
        HIPCHK(hipEventRecord(ev[EV_CHAINS_END], s));
        // optimistic, as run_chains(): the statistics are queued right behind the passes; the host only looks at the flags (pinned
        // memory the kernels wrote) when the queue has drained; in the rare round that needs more passes the statistics are redone
        // (save_gamma too: the passes launched up front almost always suffice)
        bool signalled = false;
        if (first_round) signalled = enqueue_stats(poll ? done_epoch + 1 : 0);
        else stats_enqueued = false;
        done_covers_stats = stats_enqueued;
        if (poll) {
            ++done_epoch;
            if (!signalled) hipLaunchKernelGGL(k_signal, dim3(1), dim3(1), 0, s, d_done_view, done_epoch);
            if (!wait_done(done_epoch)) throw std::runtime_error("the device did not signal completion");
        } else HIPCHK(hipStreamSynchronize(s));
        first_round = false;
        q = first_quiet(chf, chb, ss_launched);
        if (q < 0 && ss_launched > p0) {
            // no launched pass was quiet - but if the LAST one rewrote no end vector (every chunk that re-ran merged with its stored
            // trajectory; a pass that stores everything always sets its flag), every chunk's input is what it last ran from and the
            // next pass would skip them all: that pass is the quiet one, without having been launched
            const int L = ss_launched - 1;
            const int *ecf = h_flags + 2 * (plan.max_pass + 1), *ecb = h_flags + 3 * (plan.max_pass + 1);
            if (ecf[L] == 0 && ecb[L] == 0) q = ss_launched;
        }
        if (q >= 0 || ss_launched >= plan.max_pass) break;
        stats_enqueued = false;
        done_covers_stats = false;
        if (first_launched < 0) first_launched = ss_launched;
        ss_launch_passes(std::min(plan.max_pass, ss_launched + 3));
    }
    chains_dual = false;
    if (ss_args.dbg) {
        long long h[8];
        HIPCHK(hipMemcpy(h, d_dbg.p, sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr, "[cycles] ss pass 0, chunk 1: forward %lld shader clocks, %lld x 10 ns, %lld positions, %lld rows; backward %lld "
                "clocks, %lld x 10 ns, %lld positions, %lld rows\n", h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
    }
    if (q < 0) {
        stats_enqueued = false;
        // (the preparation kernel precedes the chains on the stream, its flag words sit in host-mapped memory, and the queue has drained)
        if (E_on_dev && dprep && dprep->span_underflow()) return false;
        throw std::runtime_error("chunk-boundary iteration did not converge");
    }
    // the flags of the first round did not certify, yet the very next pass was quiet: on this input the last working pass rewrites
    // end vectors WITHIN the tolerance - from now on the all-skip pass is launched up front again (one round instead of two)
    if (first_launched >= 0 && q == first_launched) ss_need_cert_pass = true;
    last_ss_passes = q - p0;
    last_fwd_passes = last_bwd_passes = q - p0;
    // every launched pass carried the end vectors forward (a skipped chunk copies them): they sit at the last pass's parity
    ss_warm_parity = (ss_launched - 1) & 1;
    ss_warm_valid = true;
    return true;
}

void smcpp_im::run_stats() {
    if (!stats_enqueued) enqueue_stats();
    finish_stats();
}

void smcpp_im::finish_stats() {
    if (!(estep_route.ss_active && done_covers_stats)) HIPCHK(hipStreamSynchronize(stream));      // (else: run_chains_ss saw the queue drain)
    done_covers_stats = false;
    std::memcpy(loglik.data(), h_ll, sizeof(double) * n_contigs);
    stats_enqueued = false;
}

// ---- statistics: one plan per enqueue (resolve_stats_plan), then branch launchers that only read it ----
// One rank update: k_rank_acc_wide (operand rows staged through LDS; modes 0 / 2), k_rank_acc over teams of up to four slabs of one
// reduction range that add their accumulators through LDS (teams != nullptr), or k_rank_acc with one wavefront per slab
// (nparts: partials the launch writes - teams, or slabs where teams == nullptr: StatsPlan::part_1 / part_e)
template <int MODE>
static void launch_rank_acc(AccArgs a, bool wide, const int2 *teams, size_t nparts, hipStream_t s) {
    a.teams = teams;
    const unsigned nx = (unsigned)nparts, ny = MODE == 3 ? 1u : (unsigned)(a.NB * a.NB);
    if constexpr (MODE == 0 || MODE == 2) {
        if (wide) {
            lds_limit_once<k_rank_acc_wide<MODE, 8>>();
            const dim3 grid(nx, (unsigned)(((a.Mp + 255) / 256) * ((a.Mp + 127) / 128)));
            hipLaunchKernelGGL((k_rank_acc_wide<MODE, 8>), grid, dim3(512), RW_LDS, s, a);
            return;
        }
    }
    if constexpr (MODE != 1) {
        if (teams) { hipLaunchKernelGGL((k_rank_acc<MODE, true>), dim3(nx, ny), dim3(256), 0, s, a); return; }
    }
    hipLaunchKernelGGL(k_rank_acc<MODE>, dim3(nx, ny), dim3(64), 0, s, a);
}

// deterministic reduction of slab partials: ny ranges of len values, z shares each
static void sum_parts(const double *part, const int *off, double *red, int len, unsigned ny, int z, hipStream_t s) {
    hipLaunchKernelGGL(k_sum_parts, dim3(ceil_div(len, 256), ny, z), dim3(256), 0, s, part, off, red, len, z);
}
static int fin_blocks(int Mp, int K) { return ceil_div((long long)Mp * Mp, 256) + ceil_div((long long)(K + 1) * Mp, 256); }

StatsPlan smcpp_im::resolve_stats_plan(bool generators) const {
    using P = StatsPlan;
    P p;
    p.resolved = true;
    const bool dual = dual_stream != 0;
    // the span > 1 branch (weights, rank update, span fold or U / W products, Y) does not depend on the span-1 branch (weights, rank
    // update, gamma sums): on two streams the short launches of one fill the gaps of the other
    p.split = dual && !lay.slabs_eg.h.empty();
    // Eigen-free statistics of small inputs: the span > 1 rank update -> reduction -> span fold (2 x s_max serial steps) is the critical
    // path, and a hop between two streams costs ~10 us (2 us between two kernels of one queue): THAT branch keeps the main stream,
    // directly behind the chains and in front of the finalisation, and the span-1 branch (which has slack) forks.  (M > 64: chip-filling
    // rank updates, the hops do not matter and the other order is 3 % faster.)
    const bool crit_main = estep_route.eigfree && p.split && lay.n_e_rows < 1000000 && Mp <= 64;
    p.span_gt1 = p.split && !crit_main ? P::SECOND : P::MAIN;
    p.span1 = crit_main ? P::SECOND : P::MAIN;
    // M <= 64, from half a million span-1 rows on: ONE pass over the key-sorted span-1 rows gives the rank update and the key's gamma
    // sums from the same operands (k_rank_acc<3>): whole genome (3.6 M rows, bandwidth-bound) 3.77 -> 3.15 ms of statistics; one 100
    // Mbp contig (129 k rows, latency-bound) 0.208 -> 0.225 ms - there the gamma sums stay a third concurrent branch, unless the span > 1
    // branch holds the main stream: then ONE side branch beats two (887 against 873 evals/s).  SMCPP_S1_FUSE=0 / 1 forces either form.
    p.s1_one_pass = Mp <= 64 && !save_gamma && !lay.slabs_fk.h.empty() &&
                    (opt().has(smcpp_opt::O_S1_FUSE) ? opt().i(smcpp_opt::O_S1_FUSE, 0) != 0 : (lay.n_1_rows >= 500000 || crit_main));
    // two kernels at M <= 64: k_rank_acc forms the span-1 weights itself, so the per-key gamma sums (k_s1_scalars + reduction) are a
    // third independent branch; else, on two streams, they are reduced at the tail of the span > 1 branch (which finishes earlier)
    const bool gsum_own = !p.s1_one_pass && dual && Mp <= 64 && !save_gamma && !lay.slabs_sc.h.empty();
    p.gsum_at = p.s1_one_pass ? P::GSUM_ONE_PASS : gsum_own ? P::GSUM_OWN_STREAM : p.split && !lay.slabs_sc.h.empty() ? P::GSUM_SPAN_GT1_TAIL : P::GSUM_SPAN1;
    p.gsum = gsum_own ? P::THIRD : p.span1;
    // nothing in the statistics reads log_c: the log-likelihood runs on the third stream beside both branches (0.1 ms on un-binned
    // data) - unless the span > 1 branch holds the main stream and the gamma sums the third: then at the head of the span-1 branch
    const bool ll_own = p.split && !crit_main;            // (joined at the end of the main stream)
    p.loglik = ll_own || (crit_main && p.s1_one_pass) ? P::THIRD : crit_main ? P::SECOND : P::MAIN;
    // Mp > 128: operand rows staged through LDS (k_rank_acc_wide: a workgroup per 256 x 128 block of the output instead of a wavefront
    // per 64 x 64 block; SMCPP_RANK_WIDE=0: k_rank_acc).  Teams of four slabs add their accumulators through LDS and write a quarter of
    // the partial bytes (SMCPP_STATS_TEAM=0: one partial per slab).
    const bool teams = stats_team_on();
    p.rank = Mp > 128 && !opt().off(smcpp_opt::O_RANK_WIDE) ? P::RANK_WIDE : teams ? P::RANK_TEAMS : P::RANK_PER_SLAB;
    p.teams_span1 = teams && !lay.teams_rk.h.empty();
    p.teams_one_pass = teams && !lay.teams_fk.h.empty();
    p.teams_span_gt1 = teams && estep_route.eigfree && !lay.teams_eg.h.empty();
    if (estep_route.eigfree) p.eigen = lay.slabs_eg.h.empty() ? P::EIG_NONE : estep_route.ss_active && !opt().off(smcpp_opt::O_SPAN_SCAN) ? P::EIG_FOLD_SCANS : P::EIG_FOLD_MATRIX_CORES;
    else p.eigen = NT <= 4 && !lay.slabs_eg.h.empty() ? P::EIG_GEN2 : P::EIG_CLASSIC;
    // the span fold (tens of serial steps on a few CUs) ends the longest dependency chain, so what it waits for goes FIRST and alone
    // (small inputs only: from ~10^6 span > 1 rows on, the two rank updates side by side finish sooner - whole genome 3.76 -> 3.36 ms)
    p.rank_early = estep_route.eigfree && p.split && lay.n_e_rows < 1000000;
    if (save_gamma && lay.n_e_rows > 0) {
        // long rows at 64 < M <= 256 with a structured T: eigen-power pieces + scan steps, which read the statistics' U / W products
        // (main stream, behind them); the other forms need alpha, beta and the eigensystems only: beside the statistics
        const bool pieces = gamma_pieces_fit() && generators;
        p.gamma_beside = dual && !pieces && !opt().off(smcpp_opt::O_GAMMA_SIDE);
        p.gamma = p.gamma_beside ? P::HIGH : P::MAIN;
        p.gamma_form = pieces ? P::GAMMA_PIECES : estep_route.eigfree ? P::GAMMA_SCAN : NT <= 4 ? P::GAMMA_EIG_BATCHES : P::GAMMA_EIG_ROWS;
    }
    // the finalisation signals the host itself when nothing follows it on the main stream and the launch is small: every block ends
    // with a device-scope fence and an atomic on ONE counter (1 500 contigs: 3.2 ms; beyond 128 blocks the one-thread kernel signals)
    p.fin_signals = !save_gamma && !ll_own && (long long)fin_blocks(Mp, K) * n_contigs <= 128;
    // ---- counts: what the launches put into their grids and size_stats_buffers() into the buffers ----
    p.part_1 = p.s1_one_pass ? (p.teams_one_pass ? lay.teams_fk.h.size() : lay.slabs_fk.h.size()) : (p.teams_span1 ? lay.teams_rk.h.size() : lay.slabs_rk.h.size());
    p.gpart_fk = p.s1_one_pass ? lay.slabs_fk.h.size() : 0;
    // (one M x M partial per span GROUP slab or team, one reduced matrix per bucket: not for generation 2, whose slabs mix the groups)
    if (!lay.slabs_eg.h.empty() && p.eigen != P::EIG_GEN2) {
        p.part_e = p.teams_span_gt1 ? lay.teams_eg.h.size() : lay.slabs_eg.h.size();
        p.red_e = estep_route.eigfree ? std::max<size_t>(1, lay.eb_gid.h.size()) : 0;
    }
    if (p.eigen == P::EIG_FOLD_SCANS || p.eigen == P::EIG_FOLD_MATRIX_CORES) p.fall = (size_t)n_contigs * Ke * ss_max_span;
    if (p.eigen == P::EIG_GEN2) {
        p.ek_slabs = lay.slabs_ek.h.size();
        int max_sl = 1;          // shares of the cross-slab reduction: ~32 slabs each (un-binned data: thousands of slabs on a handful of (contig, key) pairs)
        for (int ce = 0; ce < n_contigs * Ke; ++ce) max_sl = std::max(max_sl, lay.ek_slab_off.h[ce + 1] - lay.ek_slab_off.h[ce]);
        p.nsh = std::max(1, std::min(128, (max_sl + 31) / 32));
    }
    if (p.eigen == P::EIG_CLASSIC && Ke > 0) {
        int max_b = 0;           // slices of the groups of one (contig, key): enough blocks to fill the chip when there are many groups
        for (size_t ce = 0; ce + 1 < lay.ce_bucket_off.h.size(); ++ce) max_b = std::max(max_b, lay.ce_bucket_off.h[ce + 1] - lay.ce_bucket_off.h[ce]);
        p.nsl = std::max(1, std::min(std::min(256, max_b), 2048 / std::max(1, ceil_div((long long)Mp * Mp, 256) * n_contigs * Ke)));
    }
    return p;
}

// The buffers whose size follows from the plan, at the head of the statistics: a steady-state E-step finds them large enough
void smcpp_im::size_stats_buffers(const StatsPlan &p) {
    const size_t MM = (size_t)Mp * Mp;
    d_part_1.alloc(std::max<size_t>(1, p.part_1) * MM);
    d_gpart_fk.alloc(p.gpart_fk * Mp);
    if (p.part_e) d_part_e.alloc(p.part_e * MM);
    d_red_e.alloc(p.red_e * MM);
    d_Fall.alloc(p.fall * MM);
    // (generation 2, per slab: the M x M accumulator and the M diagonal sums)
    if (p.eigen == StatsPlan::EIG_GEN2) { d_part_ek.alloc(std::max<size_t>(1, p.ek_slabs) * (MM + Mp)); d_red_ek.alloc((size_t)n_contigs * Ke * p.nsh * (MM + Mp)); }
    if (p.nsl > 1) d_Zpart.alloc((size_t)p.nsl * n_contigs * Ke * MM);
}

// A side stream forks off the chains' end and waits for the parameter arena copied beside them as well: its kernels read the log-scales
// and the emission table (a wait in front of the fork event instead costs 12 us per eval: every branch then starts behind the barrier
// packet; on the side streams, which have slack, it costs nothing measurable)
void smcpp_im::fork_from_chains(hipStream_t x) {
    HIPCHK(hipStreamWaitEvent(x, ev[estep_route.ss_active ? EV_CHAINS_END : EV_STATS_FORK], 0));
    if (estep_route.arena_side) HIPCHK(hipStreamWaitEvent(x, ev[EV_ARENA], 0));
}

// weights (and, span-1 rows, partial gamma sums and save_gamma's rows) of the span-1 rows, or only the weights of the span > 1 rows
S1Args smcpp_im::s1_args(bool span_gt1) {
    S1Args a;
    a.M = M; a.Mp = Mp;
    a.nslabs = (int)(span_gt1 ? lay.slabs_eg.h.size() : lay.slabs_sc.h.size()); a.slabs = span_gt1 ? lay.slabs_eg.d.p : lay.slabs_sc.d.p;
    a.perm = span_gt1 ? lay.perme.d.p : lay.perm1.d.p;
    a.alpha = d_alpha.p; a.beta = d_beta.p; a.cnorm = d_cnorm.p; a.w1 = d_w1.p; a.gpart = d_gpart.p;
    a.gamma_rows = !span_gt1 && save_gamma ? d_gamma_rows.p : nullptr;
    a.only_w1 = span_gt1 ? 1 : 0;
    return a;
}

AccArgs smcpp_im::acc_args(const HostDev<Slab> &sl, const int *perm, const int2 *permk, double *part, double *gpart) {
    AccArgs a;
    a.M = M; a.Mp = Mp; a.NB = (Mp + 63) / 64; a.rowinfo = d_rowinfo.p; a.alpha = d_alpha.p; a.beta = d_beta.p;
    a.w1 = d_w1.p; a.cnorm = d_cnorm.p; a.E = d_E.p; a.Xs = d_Xs.p; a.Ys = d_Ys.p;
    a.nslabs = (int)sl.h.size(); a.slabs = sl.d.p; a.perm = perm; a.permk = permk; a.part = part; a.gpart = gpart; a.teams = nullptr;
    return a;
}

// weights of the span > 1 rows (M <= 64: k_rank_acc<2> forms them itself), then their rank update per (span, key) group
void smcpp_im::launch_span_gt1_rank(const StatsPlan &p) {
    const hipStream_t se = plan_stream(p.span_gt1);
    if (Mp > 64) launch_s1(NPL, s1_args(true), se);
    launch_rank_acc<2>(acc_args(lay.slabs_eg, lay.perme.d.p, nullptr, d_part_e.p, nullptr), p.rank == StatsPlan::RANK_WIDE,
                       p.teams_span_gt1 ? lay.teams_eg.d.p : nullptr, p.part_e, se);
}

void smcpp_im::launch_span1_branch(const StatsPlan &p) {
    const hipStream_t sp1 = plan_stream(p.span1), sg1 = plan_stream(p.gsum);
    const int MMi = Mp * Mp;
    if (p.gsum_at == StatsPlan::GSUM_OWN_STREAM) {
        if (p.span1 == StatsPlan::SECOND) fork_from_chains(stream3);     // (forks where the span-1 branch does)
        else hand_over(EV_GSUM_FORK, stream, stream3);
    }
    if (!p.s1_one_pass && !lay.slabs_sc.h.empty()) {
        launch_s1(NPL, s1_args(false), sg1);
        if (p.gsum_at == StatsPlan::GSUM_OWN_STREAM) {
            sum_parts(d_gpart.p, lay.gk_slab_off.d.p, d_red_g.p, Mp, n_contigs * K, 1, sg1);
            HIPCHK(hipEventRecord(ev[EV_GSUM_DONE], sg1));
        } else if (p.gsum_at == StatsPlan::GSUM_SPAN_GT1_TAIL) HIPCHK(hipEventRecord(ev[EV_S1_SCALARS], sp1));
    }
    // the span > 1 rank update launched early on the side stream: the span-1 branch waits for it only where its OWN rank update
    // starts - its weights pass (k_s1_scalars, bound by memory round trips) runs beside the head of that rank update
    if (p.rank_early && p.span1 == StatsPlan::MAIN) HIPCHK(hipStreamWaitEvent(sp1, ev[EV_RANK2_DONE], 0));
    if (p.s1_one_pass) {
        launch_rank_acc<3>(acc_args(lay.slabs_fk, lay.perm1.d.p, nullptr, d_part_1.p, d_gpart_fk.p), false,
                           p.teams_one_pass ? lay.teams_fk.d.p : nullptr, p.part_1, sp1);
        sum_parts(d_gpart_fk.p, lay.fk_gk_off.d.p, d_red_g.p, Mp, n_contigs * K, lay.ZG, sp1);
        sum_parts(d_part_1.p, p.teams_one_pass ? lay.fk_c_team_off.d.p : lay.fk_c_off.d.p, d_red_1.p, MMi, n_contigs, lay.ZS, sp1);
    } else {
        if (!lay.slabs_rk.h.empty())
            launch_rank_acc<0>(acc_args(lay.slabs_rk, lay.perm1.d.p, lay.perm1k.d.p, d_part_1.p, nullptr), p.rank == StatsPlan::RANK_WIDE,
                               p.teams_span1 ? lay.teams_rk.d.p : nullptr, p.part_1, sp1);
        if (p.gsum_at == StatsPlan::GSUM_SPAN1) sum_parts(d_gpart.p, lay.gk_slab_off.d.p, d_red_g.p, Mp, n_contigs * K, 1, sp1);
        sum_parts(d_part_1.p, p.teams_span1 ? lay.s1_team_off.d.p : lay.s1_slab_off.d.p, d_red_1.p, MMi, n_contigs, lay.ZS, sp1);
    }
    HIPCHK(hipEventRecord(ev[EV_SPAN1_DONE], sp1));
}

void smcpp_im::launch_span_gt1_branch(const StatsPlan &p, FinArgs &fa) {
    const hipStream_t se = plan_stream(p.span_gt1);
    const int MMi = Mp * Mp, nb2 = ceil_div((long long)Mp * Mp, 256);
    switch (p.eigen) {
    case StatsPlan::EIG_NONE: break;
    case StatsPlan::EIG_FOLD_SCANS:
    case StatsPlan::EIG_FOLD_MATRIX_CORES:
        // weights and rank update per (span, key) group (unless launched early), deterministic reduction of the slab partials, then
        // the span fold per (contig, key)
        if (!p.rank_early) launch_span_gt1_rank(p);
        if (!lay.eb_gid.h.empty())                                     // ONE share per bucket: k_span_F reads it on its serial path
            sum_parts(d_part_e.p, p.teams_span_gt1 ? lay.eb_team_off.d.p : lay.eb_slab_off.d.p, d_red_e.p, MMi, (unsigned)lay.eb_gid.h.size(), 1, se);
        if (p.eigen == StatsPlan::EIG_FOLD_SCANS) {
            // a row of F times A / A times a column of H is one O(M) step of the backward / forward chain operator, so one wavefront
            // per row / column walks all s_max steps on its own - no matrix product, no barrier
            const int nwav = n_contigs * Ke * M;
            const dim3 grid(ceil_div(nwav, 4)), block(256);
            switch (NPL) {
#define SC_(x) case x: hipLaunchKernelGGL((k_span_scan<x, 0>), grid, block, 0, se, ss_args, fa, ss_max_span, d_Fall.p); \
                       hipLaunchKernelGGL((k_span_scan<x, 1>), grid, block, 0, se, ss_args, fa, ss_max_span, d_Fall.p); break;
                SC_(1) SC_(2) SC_(3) SC_(4) SC_(8)
                default: SC_(16)
#undef SC_
            }
        } else {
            // strips of 16 rows (F) / columns (H), one workgroup each, F_t through scratch
            const int nstrip = NT, nwg = n_contigs * Ke * nstrip;
#define B_(x) { hipLaunchKernelGGL((k_span_big<x, 0>), dim3(nwg), dim3(64 * x), 0, se, fa, ss_max_span, d_Fall.p); \
                hipLaunchKernelGGL((k_span_big<x, 1>), dim3(nwg), dim3(64 * x), 0, se, fa, ss_max_span, d_Fall.p); }
            if (NT == 1) B_(1) else if (NT == 2) B_(2) else if (NT == 3) B_(3) else if (NT == 4) B_(4)
            else if (NT <= 8) B_(8) else if (NT <= 12) B_(12) else B_(16)
#undef B_
        }
        break;
    case StatsPlan::EIG_GEN2: {
        // slabs that mix span groups, the span-Q weighting inside the accumulation
        UWArgs ua;
        ua.M = M; ua.Mp = Mp; ua.nslabs = (int)p.ek_slabs; ua.slabs = lay.slabs_ek.d.p; ua.perm = lay.perme.d.p;
        ua.alpha = d_alpha.p; ua.beta = d_beta.p; ua.g_eig = d_g_eig.p; ua.g_scale = d_g_scale.p;
        ua.dpow = d_dpow.p; ua.PinvT = d_PinvT.p; ua.Prm = d_Prm.p; ua.Xs = nullptr; ua.Ys = nullptr;
        ua.pos_gid = lay.epos_gid.d.p; ua.g_span = d_g_span.p;
        const int nce = n_contigs * Ke;
        const int LEN = MMi + Mp, nsh = p.nsh;          // per slab: the M x M accumulator and the M diagonal sums
        const int nblk = ceil_div(ua.nslabs, 4);
        const size_t shm = (size_t)2 * (16 * NT) * (16 * NT + 1) * sizeof(double);
        switch (NT) {
#define F_(x) case x: lds_limit_once<k_eig_fused2<x>>(); hipLaunchKernelGGL(k_eig_fused2<x>, dim3(nblk), dim3(256), shm, se, ua, d_part_ek.p); break;
            F_(1) F_(2) F_(3)
            default: F_(4)
#undef F_
        }
        sum_parts(d_part_ek.p, lay.ek_slab_off.d.p, d_red_ek.p, LEN, (unsigned)nce, nsh, se);
        hipLaunchKernelGGL(k_fin_Z2, dim3(nb2, nce), dim3(256), 0, se, fa, (const double *)d_red_ek.p, nsh);
        hipLaunchKernelGGL(k_fin_Y, dim3(nb2, nce), dim3(256), 0, se, fa);
        break;
    }
    case StatsPlan::EIG_CLASSIC:
        if (!lay.slabs_eg.h.empty()) {
            UWArgs ua;
            ua.M = M; ua.Mp = Mp; ua.nslabs = (int)lay.slabs_eg.h.size(); ua.slabs = lay.slabs_eg.d.p; ua.perm = lay.perme.d.p;
            ua.alpha = d_alpha.p; ua.beta = d_beta.p; ua.g_eig = d_g_eig.p; ua.g_scale = d_g_scale.p;
            ua.dpow = d_dpow.p; ua.PinvT = d_PinvT.p; ua.Prm = d_Prm.p; ua.Xs = d_Xs.p; ua.Ys = d_Ys.p; ua.pos_gid = nullptr; ua.g_span = nullptr;
            launch_uw(NT, ua, se);
            // (no reduction pass over the slab partials: k_fin_Z sums the slabs of a bucket itself)
            launch_rank_acc<1>(acc_args(lay.slabs_eg, lay.perme.d.p, nullptr, d_part_e.p, nullptr), false, nullptr, p.part_e, se);
        }
        if (Ke > 0) {
            const int nsl = p.nsl;
            fa.Zpart = nsl > 1 ? d_Zpart.p : nullptr;
            hipLaunchKernelGGL(k_fin_Z, dim3(nb2, n_contigs * Ke, nsl), dim3(256), 0, se, fa);
            if (nsl > 1) hipLaunchKernelGGL(k_fin_Zsum, dim3(nb2, n_contigs * Ke), dim3(256), 0, se, fa, nsl, n_contigs * Ke);
            hipLaunchKernelGGL(k_fin_Y, dim3(nb2, n_contigs * Ke), dim3(256), 0, se, fa);
        }
        break;
    }
}

void smcpp_im::launch_gamma_rows(const StatsPlan &p) {
    const hipStream_t sg = plan_stream(p.gamma);
    const int nb2 = ceil_div((long long)Mp * Mp, 256);
    GammaRowArgs ga;
    ga.M = M; ga.Mp = Mp; ga.nrows = (int)lay.n_e_rows; ga.perm = lay.perme.d.p; ga.row_slab = lay.erow_slab.d.p;
    ga.slabs = lay.slabs_eg.d.p; ga.g_eig = d_g_eig.p; ga.g_span = d_g_span.p; ga.dun = d_dun.p; ga.dsc = d_dsc.p; ga.dpow = d_dpow.p;
    ga.Prm = d_Prm.p; ga.Pinvrm = d_Pinvrm.p; ga.PinvT = d_PinvT.p; ga.Sq = nullptr;
    ga.alpha = d_alpha.p; ga.beta = d_beta.p; ga.gamma_rows = d_gamma_rows.p; ga.erow_desc = lay.erow_desc.d.p;
    switch (p.gamma_form) {
    case StatsPlan::GAMMA_NONE: break;
    case StatsPlan::GAMMA_PIECES: {
        // long rows at 64 < M <= 256: eigen-power pieces + scan steps (chains_ss.hpp: k_piece_vectors)
        build_gamma_pieces();
        const int MS = 64 * NPL;
        gp.gen.upload(ss_gen, sg);
        gp.cs.alloc((size_t)Ke * 2 * Mp);
        gp.l2d.alloc((size_t)Ke * Mp);
        const size_t npc = gp.pieces.h.size();
        gp.pvf.alloc(npc * Mp); gp.pvb.alloc(npc * Mp); gp.pgam.alloc(npc * Mp);
        PieceArgs pa;
        pa.M = M; pa.Mp = Mp; pa.npieces = (int)npc; pa.ntiles = (int)gp.tiles.h.size();
        pa.pieces = gp.pieces.d.p; pa.tiles = gp.tiles.d.p; pa.Xs = d_Xs.p; pa.Ys = d_Ys.p; pa.dsc = d_dsc.p;
        pa.PT = d_PT.p; pa.Pinvrm = d_Pinvrm.p; pa.cs = gp.cs.p; pa.l2d = gp.l2d.p; pa.pvf = gp.pvf.p; pa.pvb = gp.pvb.p; pa.pgam = gp.pgam.p;
        hipLaunchKernelGGL(k_piece_rowsums, dim3(ceil_div(Ke * 2 * Mp, 256)), dim3(256), 0, sg, Ke, Mp, (const double *)d_PT.p,
                           (const double *)d_Pinvrm.p, gp.cs.p, (const double *)d_dsc.p, gp.l2d.p);
        if (pa.ntiles > 0) {
            lds_limit_once<k_piece_vectors>();
            const size_t shm = (size_t)4 * 16 * (Mp + 4) * sizeof(double);
            const int nblk = std::min(2 * ceil_div(pa.ntiles, 4), 2048);
            hipLaunchKernelGGL(k_piece_vectors, dim3(nblk), dim3(256), shm, sg, pa);
        }
        SsArgs sa = SsArgs();
        sa.M = M; sa.Mp = Mp;
        set_generators(sa, gp.gen.p, MS, ss_c0);
        const int nw = (int)std::min<size_t>(npc, 4096);
        d_gpark.alloc((size_t)nw * 64 * MS);
        const dim3 grid(ceil_div(nw, 4)), block(256);
        switch (NPL) {
#define GP_(x) case x: hipLaunchKernelGGL((k_gamma_rows_scan<x, true>), grid, block, 0, sg, sa, ga, (const RowInfo *)d_rowinfo.p, \
                                          (const double *)d_E.p, d_gpark.p, 64, nw, pa); break;
            GP_(2) GP_(3)
            default: GP_(4)
#undef GP_
        }
        hipLaunchKernelGGL(k_gamma_merge_pieces, dim3((unsigned)ceil_div((long long)lay.n_e_rows * Mp, 256)), dim3(256), 0, sg, Mp, (int)lay.n_e_rows,
                           (const int *)gp.pfirst.d.p, (const GPiece *)gp.pieces.d.p, (const double *)gp.pgam.p, d_gamma_rows.p);
        break;
    }
    case StatsPlan::GAMMA_SCAN: {
        // no eigensystem on this path: 2 span - 1 scan steps per row, one (persistent) wavefront per row, the forward vectors parked
        // as floats in the wavefront's piece of a scratch buffer
        const int nw = (int)std::min<long long>((long long)lay.n_e_rows, NPL >= 8 ? 1024 : 4096);
        d_gpark.alloc((size_t)nw * ss_max_span * 64 * NPL);
        const dim3 grid(ceil_div(nw, 4)), block(256);
        switch (NPL) {
#define GS_(x) case x: hipLaunchKernelGGL((k_gamma_rows_scan<x>), grid, block, 0, sg, ss_args, ga, (const RowInfo *)d_rowinfo.p, \
                                          (const double *)d_E.p, d_gpark.p, ss_max_span, nw); break;
            GS_(1) GS_(2) GS_(3) GS_(4) GS_(8)
            default: GS_(16)
#undef GS_
        }
        break;
    }
    case StatsPlan::GAMMA_EIG_BATCHES: {
        // one launch per (contig, eigen key): a workgroup shares one LDS copy of P, Pinv and the reciprocal eigenvalue differences
        // (NT > 2: the reciprocal differences live in registers and the fold tile is half as wide - four wavefronts fit as well)
        const int NW = 4;
        const size_t shm2 = (size_t)((NT <= 2 ? 3 : 2) * Mp * (Mp + 1) + NW * (2 * 16 * (Mp + 1) + Mp * (NT <= 2 ? 17 : 9) + Mp) + Mp) * sizeof(double);
        for (int ce = 0; ce < n_contigs * Ke; ++ce) {
            const int q0 = lay.ce_row_off[ce], q1 = lay.ce_row_off[ce + 1];
            if (q1 <= q0) continue;
            const int nbatch = std::max(1, std::min(4, (q1 - q0 + 16 * NW * 2048 - 1) / (16 * NW * 2048)));   // batches of 16 rows per wavefront
            const int nblk = ceil_div(q1 - q0, 16 * NW * nbatch);
            switch (NT) {
#define G_(x) case x: lds_limit_once<k_gamma_rows_b<x>>(); hipLaunchKernelGGL(k_gamma_rows_b<x>, dim3(nblk), dim3(256), shm2, sg, ga, q0, q1, ce % Ke, nbatch); break;
                G_(1) G_(2) G_(3)
                default: G_(4)
#undef G_
            }
        }
        break;
    }
    case StatsPlan::GAMMA_EIG_ROWS:
        // (M > 64: the scalar kernel on a span-Q table in memory)
        d_Sq.alloc((size_t)G * Mp * Mp);
        hipLaunchKernelGGL(k_span_q, dim3(nb2, G), dim3(256), 0, sg, M, Mp, G, (const int *)d_g_span.p,
                           (const int *)d_g_eig.p, (const double *)d_dsc.p, (const double *)d_dpow.p, d_Sq.p);
        ga.Sq = d_Sq.p;
        hipLaunchKernelGGL(k_gamma_rows_eig, dim3((unsigned)lay.n_e_rows), dim3(256), (size_t)(3 * Mp + 256) * sizeof(double), sg, ga);
        break;
    }
    if (p.gamma_beside) hand_over(EV_GAMMA_DONE, sg, stream);
}

bool smcpp_im::enqueue_stats(int signal_epoch) {
    // (whether T has generators is the one question with a side effect - ss_gen, a lazy T expanded: asked here, only where the plan depends on it)
    const StatsPlan &p = stats_plan = resolve_stats_plan(gamma_pieces_fit() && (estep_route.ss_active || ss_generators_only()));
    size_stats_buffers(p);
    const hipStream_t s = stream, sl = plan_stream(p.loglik);
    if (h_ll_cap < n_contigs) {
        if (h_ll) (void)hipHostFree(h_ll);
        h_ll_cap = n_contigs;
        HIPCHK(hipHostMalloc((void **)&h_ll, sizeof(double) * h_ll_cap, hipHostMallocCoherent | hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer((void **)&d_ll_view, h_ll, 0));
    }
    // the parameter arena of a lean E-step (Td, the emission table of a set_raw manager, the groups' log-scales) is copied on the
    // second stream beside the chains (EstepRoute::arena_side); every stream of the statistics waits for it
    if (estep_route.arena_side) HIPCHK(hipStreamWaitEvent(s, ev[EV_ARENA], 0));
    if (save_gamma) {
        d_gamma_rows.alloc((size_t)total_rows * Mp);
        // Every row 1 .. L of a contig is written whole by the statistics (span-1 rows: k_s1_scalars; span > 1 rows: the per-row gamma
        // kernels); only row 0 (column 0 comes from gamma0) is nobody's: it alone is cleared.  (A memset of the whole buffer here,
        // behind the fork event, could wipe rows the span-1 branch on its side stream had already written.)
        for (int c = 0; c < n_contigs; ++c)
            HIPCHK(hipMemsetAsync(d_gamma_rows.p + (size_t)contig_base[c] * Mp, 0, sizeof(double) * Mp, s));
        if (p.gamma_beside) hand_over(EV_GAMMA_FORK, s, stream_hi);
    }
    // ---- fork ----
    if (p.split) {
        if (!estep_route.ss_active) HIPCHK(hipEventRecord(ev[EV_STATS_FORK], s));
        fork_from_chains(stream2);
    }
    // ---- log-likelihood (also materialises log_c per row) ----
    LoglikArgs la;
    la.cnorm = d_cnorm.p; la.rowinfo = d_rowinfo.p; la.g_logscale = d_g_logscale.p;
    la.contig_base = d_contig_base.p; la.contig_L = d_contig_L.p; la.partial = d_llpart.p; la.loglik = d_loglik.p;
    la.logc = d_logc.p; la.nblk = lay.llblk;
    la.loglik_host = d_ll_view;          // the final kernel writes the per-contig values into the pinned array as well: no copy
    if (estep_route.ss_active && h_done) {
        // (h_done[8]: beside the completion word, cleared here - nothing of an earlier E-step or round is in flight when the host enqueues)
        h_done[8] = 0;
        la.g_span = d_g_span.p; la.hyb_th = plan.hybrid ? plan.hyb_th : 0x7fffffff; la.range_flag = d_done_view + 8;
    }
    if (p.loglik == StatsPlan::THIRD) fork_from_chains(sl);
    hipLaunchKernelGGL(k_loglik_partial, dim3(lay.llblk, n_contigs), dim3(256), 0, sl, la);
    hipLaunchKernelGGL(k_loglik_final, dim3(n_contigs), dim3(256), 0, sl, la);
    if (p.loglik == StatsPlan::THIRD) HIPCHK(hipEventRecord(ev[EV_LOGLIK_DONE], sl));
    FinArgs fa;
    fa.M = M; fa.Mp = Mp; fa.K = K; fa.G = G; fa.Ke = Ke; fa.n_contigs = n_contigs;
    fa.eb_slab_off = lay.eb_slab_off.d.p; fa.eb_gid = lay.eb_gid.d.p; fa.ce_bucket_off = lay.ce_bucket_off.d.p;
    fa.s1_slab_off = lay.s1_slab_off.d.p; fa.gk_slab_off = lay.gk_slab_off.d.p; fa.g_span = d_g_span.p;
    fa.e_kid = d_e_kid.p; fa.dsc = d_dsc.p; fa.dun = d_dun.p; fa.Prm = d_Prm.p; fa.Pinvrm = d_Pinvrm.p;
    fa.E = d_E.p; fa.Td = d_Td.p; fa.ZS = lay.ZS; fa.red_e = nullptr; fa.red_1 = d_red_1.p; fa.red_g = d_red_g.p; fa.ZG = p.s1_one_pass ? lay.ZG : 1;
    fa.alpha = d_alpha.p; fa.beta = d_beta.p; fa.contig_base = d_contig_base.p;
    fa.Z = d_Z.p; fa.Y = d_Y.p; fa.xisum = d_xisum.p; fa.gsum = d_gsum.p; fa.gamma0 = d_gamma0.p;
    fa.dpow = d_dpow.p;
    fa.part_e = p.part_e ? d_part_e.p : nullptr;
    if (p.red_e) fa.red_e = d_red_e.p;
    fa.eigfree = estep_route.eigfree ? 1 : 0;
    // ---- the two branches ----
    if (p.rank_early) {
        launch_span_gt1_rank(p);
        if (p.span1 == StatsPlan::MAIN) HIPCHK(hipEventRecord(ev[EV_RANK2_DONE], plan_stream(p.span_gt1)));
    }
    launch_span1_branch(p);
    launch_span_gt1_branch(p, fa);
    if (p.gsum_at == StatsPlan::GSUM_SPAN_GT1_TAIL) {
        HIPCHK(hipStreamWaitEvent(plan_stream(p.span_gt1), ev[EV_S1_SCALARS], 0));
        sum_parts(d_gpart.p, lay.gk_slab_off.d.p, d_red_g.p, Mp, n_contigs * K, 1, plan_stream(p.span_gt1));
    }
    // ---- joins: the main stream waits for ONE event of the second stream (every wait is a barrier packet of a few microseconds on
    // the queue it is put on, signalled or not); the third stream joins through the second where that carries the span-1 branch ----
    if (p.split) {
        if (p.loglik == StatsPlan::THIRD && p.span1 == StatsPlan::SECOND) HIPCHK(hipStreamWaitEvent(stream2, ev[EV_LOGLIK_DONE], 0));
        hand_over(EV_SIDE_DONE, stream2, s);
    }
    if (p.gsum_at == StatsPlan::GSUM_OWN_STREAM) HIPCHK(hipStreamWaitEvent(s, ev[EV_GSUM_DONE], 0));
    // ---- finalisation ----
    const int nb2 = ceil_div((long long)Mp * Mp, 256), nbf = fin_blocks(Mp, K);
    const bool signals = signal_epoch != 0 && p.fin_signals;
    if (signals) {
        if (!d_fin_ctr.p) { d_fin_ctr.alloc(1); HIPCHK(hipMemsetAsync(d_fin_ctr.p, 0, sizeof(unsigned), s)); fin_target = 0; }
        fin_target += (unsigned)nbf * (unsigned)n_contigs;
    }
    hipLaunchKernelGGL(k_fin_both, dim3(nbf, n_contigs), dim3(256), 0, s, fa, nb2, d_fin_ctr.p, fin_target,
                       signals ? d_done_view : (int *)nullptr, signal_epoch);
    // ---- per-row gammas ----
    launch_gamma_rows(p);
    HIPCHK(hipGetLastError());
    if (p.loglik == StatsPlan::THIRD && p.span1 == StatsPlan::MAIN) HIPCHK(hipStreamWaitEvent(s, ev[EV_LOGLIK_DONE], 0));
    HIPCHK(hipEventRecord(ev[EV_STATS_DONE], s));
    stats_enqueued = true;
    return signals;
}

// The pieces of the eigen rows (chains_ss.hpp: k_piece_vectors): at most 64 positions each, in the order of the sorted eigen-row
// permutation (so the pieces of one (contig, eigen key) are contiguous and a row's pieces are in position order); tiles of sixteen
// pieces of ONE eigen key that need an interpolated vector (every piece of a row that has more than one).
void smcpp_im::build_gamma_pieces() {
    if (gp.built) return;
    constexpr int PL = 64;
    gp.pfirst.h.reserve(lay.perme.h.size() + 1);
    GTile cur; cur.es = -1; cur.cnt = 0;
    auto flush = [&]() { if (cur.cnt > 0) { for (int k = cur.cnt; k < 16; ++k) cur.pid[k] = cur.pid[cur.cnt - 1]; gp.tiles.h.push_back(cur); } cur.cnt = 0; };
    for (size_t q = 0; q < lay.perme.h.size(); ++q) {
        const Slab &sl = lay.slabs_eg.h[lay.erow_slab.h[q]];
        const Group &gr = groups[sl.aux];
        const long long row = sl.base + lay.perme.h[q];
        gp.pfirst.h.push_back((int)gp.pieces.h.size());
        const int np = (gr.span + PL - 1) / PL;
        for (int j = 0; j < np; ++j) {
            GPiece pc;
            pc.row = row; pc.q = (int)q; pc.o0 = j * PL; pc.len = std::min(PL, gr.span - j * PL); pc.span = gr.span; pc.kid = gr.kid; pc.es = gr.eig;
            if (np > 1) {
                if (cur.es != gr.eig || cur.cnt == 16) flush();
                cur.es = gr.eig;
                cur.pid[cur.cnt++] = (int)gp.pieces.h.size();
            }
            gp.pieces.h.push_back(pc);
        }
    }
    flush();
    gp.pfirst.h.push_back((int)gp.pieces.h.size());
    gp.pieces.d.upload(gp.pieces.h, stream);
    gp.tiles.d.upload(gp.tiles.h, stream);
    gp.pfirst.d.upload(gp.pfirst.h, stream);
    gp.built = true;
}

// Event intervals of the last E-step -> timing[] (lazily: see estep)
void smcpp_im::resolve_timing() {
    if (!timing_pending) return;
    timing_pending = false;
    HIPCHK(hipSetDevice(device));
    (void)hipEventSynchronize(ev[EV_STATS_DONE]);
    float f_ms = 0, b_ms = 0, s_ms = 0, fin_ms = 0;
    if (estep_route.ss_active) {
        // one launch per pass for both directions, timed below
    } else if (chains_dual) {
        (void)hipEventElapsedTime(&f_ms, ev[EV_CHAINS_START], ev[EV_FWD_END]);   // forward passes (main stream)
        (void)hipEventElapsedTime(&b_ms, ev[EV_BWD_START], ev[EV_CHAINS_END]);   // backward passes (second stream), overlapping the forward ones
    } else {
        (void)hipEventElapsedTime(&f_ms, ev[EV_CHAINS_START], ev[EV_BWD_START]);
        (void)hipEventElapsedTime(&b_ms, ev[EV_BWD_START], ev[EV_CHAINS_END]);
    }
    float chains_ms = 0;
    if (estep_route.ss_active) {
        // every pass of both directions between two events: EV_FIRST_PASS in front of the first launch, EV_CHAINS_END behind the last
        // one (a rare round that needs more passes than were launched up front includes the host's look at the flags)
        (void)hipEventElapsedTime(&chains_ms, ev[EV_FIRST_PASS], ev[EV_CHAINS_END]);
        f_ms = b_ms = chains_ms;
    } else (void)hipEventElapsedTime(&chains_ms, ev[EV_CHAINS_START], ev[EV_CHAINS_END]);
    if (prepass_launched) {
        // pass 0 ran before EV_CHAINS_START (concurrently with the host eigensolve): add its kernel intervals
        (void)hipEventElapsedTime(&pre_f_ms, ev[EV_FIRST_PASS], ev[EV_PRE_FWD_END]);
        (void)hipEventElapsedTime(&pre_b_ms, ev[EV_PRE_BWD_START], ev[EV_PRE_BWD_END]);
        f_ms += pre_f_ms; b_ms += pre_b_ms;
        chains_ms += std::max(pre_f_ms, pre_b_ms);
    }
    (void)hipEventElapsedTime(&s_ms, ev[EV_CHAINS_END], ev[EV_SPAN1_DONE]);
    (void)hipEventElapsedTime(&fin_ms, ev[EV_SPAN1_DONE], ev[EV_STATS_DONE]);
    (void)hipGetLastError();      // an interval over an event this E-step never recorded must not surface in the next launch check
    timing[0] = t_host01;
    timing[1] = chains_ms;   // wall time of both chains (they overlap in dual-stream mode)
    timing[2] = f_ms; timing[3] = b_ms; timing[4] = s_ms; timing[5] = fin_ms;
    timing[6] = t_host12;
    timing[7] = last_fwd_passes; timing[8] = last_bwd_passes;
}

// structured_T: what ss_extract_generators() found; in front of it plan.scan, "not disproved yet" - then only the first refusal can fire.
EstepRoute smcpp_im::resolve_estep_route(bool structured_T, bool underflow) const {
    EstepRoute r;
    // span > 1 rows without an eigensystem (k_span_fold); with save_gamma their per-row posteriors come from scan steps too (k_gamma_rows_scan)
    r.eigfree_static = !opt().off(smcpp_opt::O_EIGFREE) && Mp <= 1024 && ss_max_span <= 64 && (!save_gamma || !opt().off(smcpp_opt::O_GAMMA_SCAN));
    r.ss_active = structured_T;
    r.eigfree = r.ss_active && r.eigfree_static;
    if (Mp > 256 && !(plan.scan && r.eigfree_static))
        r.refuse = "more than 256 hidden states: only the scan chains with eigen-free statistics are built (rows longer than 64 positions are cut "
                   "into pieces at construction unless SMCPP_SPLIT_SPANS=0 / SMCPP_EIGFREE=0 forbid it or the pieces would not fit the device)";
    else if (Mp > 256 && !r.ss_active && underflow)
        r.refuse = "more than 256 hidden states: an emission entry is too small for the scan chains, which take a row of span s in s steps "
                   "without rescaling (on a row of span s > 1, s x log(smallest entry of its key's emission vector) < -450 or s x log(largest "
                   "entry) < -80; the transition matrix has the structure they need, and the dense fallback kernels stop at 256)";
    else if (Mp > 256 && !r.ss_active)
        r.refuse = "more than 256 hidden states: the transition matrix must have the structure of the reference's "
                   "HJTransition (the dense fallback kernels stop at 256)";
    r.host_E = E_on_dev && !r.eigfree;       // only the lean path reads a device-prepared table from HBM alone (its kernel checks the underflow bound)
    r.arena_side = r.eigfree && dual_stream; // lean E-steps copy the (small) parameter arena on stream2 beside the chains (EV_ARENA)
    return r;
}

void smcpp_im::estep(bool redo) {
    if (std::isnan(theta) || std::isnan(rho) || std::isnan(alpha))
        throw std::runtime_error("theta / rho / alpha must be set");
    if (!redo) { estep_redone = false; estep_redone_why = ""; }
    HIPCHK(hipSetDevice(device));
    timing_pending = false;          // (intervals nobody asked for: the events are about to be recorded again)
    auto t0 = std::chrono::steady_clock::now();
    HostTrace tr;
    prepare_params();
    tr.mark("estep: prepare_params");
    host_timing[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((int)pi.size() != M || (!T_lazy && (int)T.size() != M * M) || (!E_on_dev && (int)E.size() != K * M))
        throw std::runtime_error("parameters are not set");
    if (opt().poison_nan && save_gamma) {
        // SMCPP_DEBUG_POISON=nan: the per-row posteriors (padding columns included) are NaN again on every save_gamma E-step - on the
        // main stream in front of everything this E-step enqueues, not behind the chains' fork event (the round-6 race below,
        // enqueue_stats): a row or column no statistics kernel writes shows up as NaN instead of as the previous E-step's value.
        // Row 0 of each contig is cleared again by enqueue_stats.
        d_gamma_rows.alloc((size_t)total_rows * Mp);
        HIPCHK(hipMemsetAsync(d_gamma_rows.p, 0xff, sizeof(double) * d_gamma_rows.n, stream));
    }
    HIPCHK(hipEventRecord(ev[EV_ESTEP], stream));
    EstepRoute er = resolve_estep_route(plan.scan);                  // in front of the generators: T may have the structure
    if (er.refuse) throw std::runtime_error(er.refuse); if (er.host_E) sync_host_E();
    const bool structured = plan.scan && ss_extract_generators();     // ... and with what they say about T (and, of a host table, the bound)
    er = resolve_estep_route(structured, plan.scan && ss_underflow);
    if (er.refuse) throw std::runtime_error(er.refuse); if (er.host_E) sync_host_E();       // (refused: estep_route stays the last E-step's)
    estep_route = er;
    if (plan.scan && !er.ss_active && ss_underflow && g_logger_cb)
        log_msg("WARNING", "E-step: the scan chains are refused on these parameters (%s): chain family %d instead of %d",
                ss_range_refused ? "a row's evidence left the range of their float intermediates" : "an emission entry is too small for a row's span",
                (int)plan.dense, plan.hybrid ? 6 : 5);
    tr.mark("estep: extract generators");
    prepass_launched = false;
    if (!estep_route.ss_active) { ss_warm_valid = false; stage_static_and_prepass(); }   // (when eligible) pass 0 of both chains starts now, on eigen-free operands
    else { static_packed = false; if (!plan.hybrid) ss_launch_initial(); }               // the chains need no eigensystem: they start now
    tr.mark("estep: first launches");
    host_prep_and_upload();   // the reference rebuilds the eigensystems on every E-step (inference_manager.cpp:112)
    tr.mark("estep: host_prep_and_upload");
    if (estep_route.ss_active && plan.hybrid) ss_launch_initial();       // hybrid rows read the eigensystems: the chains start behind them
    auto t1 = std::chrono::steady_clock::now();
    bool chains_ok = true;
    if (estep_route.ss_active) chains_ok = run_chains_ss(); else run_chains();
    tr.mark("estep: chains (host view)");
    if (chains_ok) run_stats();
    tr.mark("estep: statistics enqueued");
    if (E_on_dev) {
        dprep->check_flags();
        if (estep_route.ss_active && dprep->span_underflow()) {
            // an emission entry so small that `span` scan steps underflow (ss_extract_generators' bound, evaluated by the kernel
            // that formed the table): this E-step is redone on the dense kernels from the host copy of the same parameters - whether
            // the chains' attempt converged on that table or not (run_chains_ss).  The second entry finds the table on the host, so
            // the host bound sends it to the dense kernels (or, beyond 256 states, to the refusal that names the bound).
            sync_host_E();
            estep_redone = true;
            estep_redone_why = "device preparation: an emission entry is too small for `span` scan steps without rescaling (span x log(smallest entry) < -450 "
                               "or span x log(largest entry) < -80)";
            estep(true);
            return;
        }
    }
    if (estep_route.ss_active && h_done && h_done[8]) {
        // the bounds are necessary, not sufficient - a row's evidence depends on the data: the log-likelihood kernel found a scanned
        // row whose evidence left the range of the scan steps' float intermediates (kernels.hpp: LoglikArgs::range_flag), so what
        // the chains and the statistics computed cannot be trusted.  Redone on the dense kernels; remembered until the parameters change.
        sync_host_E();
        ss_range_refused = true;
        estep_redone = true;
        estep_redone_why = "scan chains: the evidence of a row of span > 1 is too small for `span` scan steps without rescaling (|log c| > 80 "
                           "or not finite)";
        estep(true);
        return;
    }
    auto t2 = std::chrono::steady_clock::now();
    // the event intervals are read when somebody asks for them (smcpp_last_timing, the debug log): EV_STATS_DONE sits BEHIND the
    // completion word the host has just seen, so querying it here would mean waiting for it
    t_host01 = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t_host12 = std::chrono::duration<double, std::milli>(t2 - t1).count();
    host_timing[3] = t_host01;
    timing_pending = true;
    if (g_logger_cb) {
        resolve_timing();
        log_msg("DEBUG", "E-step: %d contig(s), %lld rows, M = %d, K = %d keys; host %.3f ms, chains %.3f ms (%d forward / %d "
                "backward passes), statistics %.3f ms; loglik[0] = %.10g", n_contigs, total_rows - n_contigs, M, K, timing[0],
                timing[1], last_fwd_passes, last_bwd_passes, timing[4] + timing[5], loglik.empty() ? 0.0 : loglik[0]);
    }
    stats_on_host = false;
    have_reduced = false;
    if (qdev) qdev->stats_ready = false;
    gamma_valid = save_gamma;
    estep_done = true;
    dirty = false;
    sc_tab_valid = sv_tab_valid = false;   // (the score track's tables belong to the parameters of the E-step before)
}

void smcpp_im::fetch_stats() {
    if (stats_on_host) return;
    if (!estep_done) {
        // the statistics of a freshly constructed HMM (hmm.cpp:8-29): xisum = 0, gamma = 0 and per key the positions it
        // covers weighted by the default model's initial distribution - what Q() sees before the first E-step (the
        // reference derives its regularisation weight from exactly that value, smcpp/analysis/analysis.py:120-125)
        h_xisum.assign((size_t)n_contigs * M * M, 0.0);
        h_gamma0.assign((size_t)n_contigs * M, 0.0);
        h_gsum.assign((size_t)n_contigs * K * M, 0.0);
        for (int c = 0; c < n_contigs; ++c)
            for (int k = 0; k < K; ++k)
                for (int i = 0; i < M; ++i)
                    h_gsum[((size_t)c * K + k) * M + i] = span_sum[(size_t)c * K + k] * pi_default[i];
        stats_on_host = true;
        return;
    }
    HIPCHK(hipSetDevice(device));
    std::vector<double> x((size_t)n_contigs * Mp * Mp), g((size_t)n_contigs * K * Mp), g0((size_t)n_contigs * Mp);
    HIPCHK(hipMemcpy(x.data(), d_xisum.p, x.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g.data(), d_gsum.p, g.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(g0.data(), d_gamma0.p, g0.size() * sizeof(double), hipMemcpyDeviceToHost));
    h_xisum.assign((size_t)n_contigs * M * M, 0.0);
    h_gsum.assign((size_t)n_contigs * K * M, 0.0);
    h_gamma0.assign((size_t)n_contigs * M, 0.0);
    for (int c = 0; c < n_contigs; ++c) {
        for (int i = 0; i < M; ++i) {
            h_gamma0[(size_t)c * M + i] = g0[(size_t)c * Mp + i];
            for (int j = 0; j < M; ++j)
                h_xisum[((size_t)c * M + i) * M + j] = x[((size_t)c * Mp + i) * Mp + j];
        }
        for (int k = 0; k < K; ++k)
            for (int i = 0; i < M; ++i)
                h_gsum[((size_t)c * K + k) * M + i] = g[((size_t)c * K + k) * Mp + i];
    }
    stats_on_host = true;
}

