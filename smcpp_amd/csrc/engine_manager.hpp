// engine_manager.hpp - part of the ONE translation unit engine.hip (included there, in order; not a standalone header):
// the manager (struct smcpp_im): observation layout, chunks, slabs, device allocation.

// How the statistics phase of an E-step is arranged: the stream of every branch and the form of every kernel family, resolved from the
// manager's shape and the switches (smcpp_im::resolve_stats_plan).  The launches only read it; smcpp_describe() reports the last one.
struct StatsPlan {
    enum Stream { MAIN, SECOND, THIRD, HIGH };          // stream, stream2, stream3, stream_hi
    enum Rank { RANK_PER_SLAB, RANK_TEAMS, RANK_WIDE };  // k_rank_acc<.>, k_rank_acc<., true>, k_rank_acc_wide (modes 0 / 2)
    enum Eigen { EIG_NONE, EIG_FOLD_SCANS, EIG_FOLD_MATRIX_CORES, EIG_GEN2, EIG_CLASSIC };
    enum Gsum { GSUM_ONE_PASS, GSUM_OWN_STREAM, GSUM_SPAN_GT1_TAIL, GSUM_SPAN1 };   // where the per-key gamma sums are reduced
    enum Gamma { GAMMA_NONE, GAMMA_SCAN, GAMMA_PIECES, GAMMA_EIG_BATCHES, GAMMA_EIG_ROWS };
    bool resolved = false, split = false;  // split: the second stream forks off the chains' end and joins before the finalisation
    Stream span_gt1 = MAIN, span1 = MAIN, gsum = MAIN, loglik = MAIN, gamma = MAIN;
    bool s1_one_pass = false;              // span-1 rows: k_rank_acc<3> (rank update + gamma sums) instead of k_s1_scalars + k_rank_acc<0>
    Rank rank = RANK_PER_SLAB;
    bool teams_span1 = false, teams_one_pass = false, teams_span_gt1 = false;   // per rank update: one partial per team of slabs
    Eigen eigen = EIG_NONE;
    bool rank_early = false;               // the span > 1 rank update goes ahead of the span-1 branch
    Gsum gsum_at = GSUM_SPAN1;
    Gamma gamma_form = GAMMA_NONE;
    bool gamma_beside = false;             // the per-row gammas run beside the statistics
    bool fin_signals = false;              // the finalisation may raise the completion word itself
    // counts a launch and an allocation both read (size_stats_buffers): partials of the span-1 rank update (per team or per slab of
    // the form that runs) and of the span > 1 one (0: none), gamma partials of the one-pass form, ranges of the span > 1 reduction,
    // scratch matrices of the span fold, slabs and shares of generation 2, slices of the classic k_fin_Z
    size_t part_1 = 0, part_e = 0, gpart_fk = 0, red_e = 0, fall = 0, ek_slabs = 0;
    int nsh = 1, nsl = 1;
};

// What the construction cuts for the statistics kernels (smcpp_im::cut_stats_layout: no HIP call): the sorted row permutations, the
// slabs over them, the ranges the reductions walk, the teams, and the sizes that belong to the same cut.  Every list with its device
// twin; upload() is the one place that copies them.  DESIGN.md section 5: field, decided from, switch.
template <class T> struct HostDev { std::vector<T> h; DevBuf<T> d; };
struct StatsLayout {
    long long n_1_rows = 0, n_e_rows = 0, pieces = 0;   // rows of span 1 / span > 1; pieces of at most 64 positions the latter fall into
    int slab_rows_1 = 0, slab_rows_e = 0;  // rows per span-1 rank slab / per span > 1 slab
    bool teams = false;                    // the slab count was aimed at one partial per team of four (SMCPP_STATS_TEAM at construction)
    int ZS = 8;                            // shares of the cross-slab reduction of the span-1 rank partials
    int ZG = 1;                            // shares of the per-key gamma-sum reduction of the one-pass span-1 form (a hot key holds most slabs)
    int llblk = 64;                        // blocks per contig of the log-likelihood reduction
    HostDev<int> perm1, perme;             // sorted permutations: span-1 rows by (contig, key), span > 1 rows by (contig, eigen key, group)
    HostDev<int2> perm1k;                  // span-1 rows in natural order: {ell, key id} (one load resolves both)
    HostDev<Slab> slabs_sc, slabs_rk, slabs_eg;   // span-1 scalar slabs, span-1 rank slabs, eigen slabs
    HostDev<int> gk_slab_off, s1_slab_off, eb_slab_off, eb_gid, ce_bucket_off, erow_slab;
    std::vector<int> ce_row_off;           // [n_contigs*Ke + 1] first position in perme of every (contig, eigen key) (host only)
    // fused span-1 statistics (M <= 64): single-key slabs over the key-sorted span-1 rows (perm1), with their ranges per contig
    // (rank partials) and per (contig, key) (gamma partials)
    HostDev<Slab> slabs_fk;
    HostDev<int> fk_c_off, fk_gk_off;
    // teams: up to four consecutive slabs of ONE reduction range share a workgroup of k_rank_acc<., true> and one partial
    HostDev<int2> teams_fk, teams_eg, teams_rk;
    HostDev<int> fk_c_team_off, eb_team_off, s1_team_off;
    // generation-2 eigen statistics (M <= 64): slabs over the sorted eigen rows of a (contig, eigen key) that MIX span groups
    HostDev<Slab> slabs_ek;
    HostDev<int> ek_slab_off, epos_gid;
    HostDev<int4> erow_desc;               // per sorted eigen-row position: {row low / high word, group, span} (k_gamma_rows_b)
    void upload(hipStream_t s) {
        auto up = [s](auto &...x) { (x.d.upload(x.h, s), ...); };
        up(slabs_sc, slabs_rk, slabs_eg, perm1, perm1k, perme, gk_slab_off, s1_slab_off, eb_slab_off, eb_gid, ce_bucket_off, erow_slab, slabs_ek,
           slabs_fk, fk_c_off, fk_gk_off, teams_fk, teams_eg, fk_c_team_off, eb_team_off, teams_rk, s1_team_off, ek_slab_off, epos_gid, erow_desc);
    }
};

// save_gamma's long rows at 64 < M <= 256 from eigen-power pieces (chains_ss.hpp: k_piece_vectors; engine_plans.hpp): the pieces, their
// tiles, the first piece of every row - built on first use - and the scratch of their kernels
struct GammaPieces {
    bool built = false;
    HostDev<GPiece> pieces; HostDev<GTile> tiles; HostDev<int> pfirst;
    DevBuf<float> pvf; DevBuf<double> pvb, pgam, cs, l2d, gen;
};

// How the chain phase is arranged for one manager and one chunking, resolved from the host layout, the switches and the device's
// compute-unit count (smcpp_im::resolve_chain_plan - no device call); cut_chunks() cuts the two chunk lists from it, the launches
// only read it, smcpp_describe() and smcpp_host_chain_plan() print it.  DESIGN.md section 5: field, decided from, switch.
struct ChainPlan {
    // the dense fallback family, by the value smcpp_chain_mode() reports: CU-cooperative (one workgroup per chunk, chains2.hpp),
    // CU-cooperative with streamed operands (64 < M <= 256), lock-step on the matrix cores (16 chunks per workgroup, chains_lock.hpp)
    enum Dense { COOPERATIVE = 2, STREAMED_OPERANDS = 3, LOCK_STEP = 4 };
    // hybrid scan chains (un-binned data): rows whose span exceeds hyb_th take ONE eigen-power step inside the scan kernel.  All four
    // eigenvector tables of every eigen key in LDS; single-direction workgroups with the two tables a direction needs (M > 32); the
    // same with only the most frequent keys' tables in LDS, the rest - COLD keys - read from L2 (three or four eigen keys)
    enum Hybrid { NONE, ALL_TABLES, DIRECTION_SPLIT, DIRECTION_SPLIT_COLD_KEYS };
    bool resolved = false;
    Dense dense = COOPERATIVE;
    bool scan = false;                     // the input takes the scan chains (chains_ss.hpp); whether T does is decided on every E-step
    Hybrid hybrid = NONE;
    int hyb_th = 0x7fffffff, nk_lds = 0, ekey_of_slot[4] = {0, 1, 2, 3}, eslot_of_key[4] = {0, 1, 2, 3};
    bool dirsplit() const { return hybrid == DIRECTION_SPLIT || hybrid == DIRECTION_SPLIT_COLD_KEYS; }
    // launch shape
    int coop_bpc = 1;                      // cooperative workgroups resident per CU the automatic chunking aims at
    int wpc = 1;                           // scan chains: wavefronts per SIMD (workgroups per CU) the chunk lists are cut for
    int wg_waves = 4;                      // wavefronts per workgroup of k_chain_ss (hybrid with two per SIMD: 8, one table copy)
    bool mid = false;                      // one state per lane, 1.35 - 12 million positions: float halo instead of light passes
    int nlds = 0;                          // key slots whose emission vectors live in LDS
    bool all_keys_in_lds = true, two_row_scans = false;        // the instantiation of k_chain_ss
    // halo pass: the first pass of the scan chains walks into every chunk from a halo (float, then fp64 positions per direction)
    bool halo = false;
    long long halo_lf = 0, halo_df = 0, halo_lb = 0, halo_db = 0;
    // chunking
    bool by_positions = false;             // the cutter: by positions with halos (scan chains, automatic) or by rows
    long long positions = 0;               // cost units of all rows (= positions unless hybrid rows are charged SS_HYB_COST)
    double fwd_share = 0.5;
    long long waves_fwd = 0, waves_bwd = 0;
    int rows_per_chunk = 0;                // by rows: rows per chunk
    std::vector<int> chunks_fwd, chunks_bwd;                   // chunks per contig of either list
    int max_chunks_per_contig = 1, max_pass = 0;
    // power jumps of the scan chains (chains_ss.hpp); jump_P = 0: never.  Per manager: a re-plan keeps them
    int jump_kid = -1, jump_P = 0;
    // eigen-free pre-pass of the dense families (chains2.hpp: k_group_powers, POWER instantiations)
    bool power_ok = false;
    int max_span_pw = 0, pw_nbits = 5, pw_npow = 4;
};

// What an E-step decides on top of the plan (smcpp_im::resolve_chain_pass): from the chunk counts, the warm start, what the
// previous E-steps learned (last_ss_passes, ss_need_cert_pass, last_fwd_passes / last_bwd_passes) and the per-E-step switches.
struct ChainPass {
    // scan chains
    bool mixed = false;                    // the scans of the stored passes in float
    int light_f = 0, light_b = 0;          // light (float, store-free) passes per direction before the full fp64 pass
    bool use_halo = false;
    int pass0 = 0;                         // a warm start numbers its passes from 1 or 2: the parity the first pass reads
    bool jump = false;                     // the launches jump
    bool cert_up_front = false;            // the all-skip certificate pass is launched with the others
    int want = 0;                          // passes launched up front
    // dense families
    bool dual = false, warm = false, coop_tab = true;
    int want_f = 0, want_b = 0, prio = 1, prio_mask = 7;
};

// Where pi / T / E come from, per prepare_params() call (resolve_param_plan: no write, no HIP call).  DESIGN.md section 5: field, decided from, switch.
struct ParamPlan {
    enum Source { NONE, RAW, ONEPOP_HOST, ONEPOP_DEVICE, TWOPOP_HOST, TWOPOP_DEVICE_BATCH } source = NONE;      // NONE: nothing prepared yet
    enum WhyHost { NOT_FORCED, SWITCH, PREP_MODE, SIZE, LITERAL_CSFS, SEEDS_TWOPOP } why_host = NOT_FORCED;     // the FIRST condition that forced the host
    bool global_keys = false, lazy_T = false, q_device_allowed = true;
};

// What an E-step decides from where the parameters live (resolve_estep_route).  eigfree: the lean E-step; host_E: the device's table comes back first
struct EstepRoute {
    bool eigfree_static = false, ss_active = false, eigfree = false, arena_side = false, host_E = false;
    const char *refuse = nullptr;
};

struct smcpp_im {
    // ---- static problem description -------------------------------------------------------------------------
    int npop = 1, keylen = 3, M = 0, Mp = 0, NPL = 1, NT = 1, n_contigs = 0, K = 0, G = 0, Ke = 0;
    int n[2] = {0, 0}, na[2] = {2, 0};
    double polarization_error = 0.5;
    std::vector<double> hs;
    std::unique_ptr<smcpp_host::TwoPopPrep> twopop_prep;     // two-population preparation (key -> tensor-bin tables cached inside)
    std::unique_ptr<TwoPopDevCsfs> twopop_dev;               // ... its two batched conditioned-SFS problems on the device (values only)
    std::vector<int> keys;                 // [K][keylen], lexicographic
    std::vector<int> Ls;
    std::vector<long long> contig_base;    // row index of ell = 0 of each contig
    long long total_rows = 0;              // sum (L+1)
    std::vector<RowInfo> rowinfo;          // host copy
    std::vector<Group> groups;             // sorted by (eig/kid, span)
    std::vector<int> eig_kid;              // [Ke]
    std::vector<int> eig_of_key;           // [K]
    std::vector<unsigned char> present;    // [n_contigs][K] key occurs in contig
    std::vector<double> span_sum;          // [n_contigs][K] positions covered by the key in the contig
    std::vector<double> pi_default;        // [M] initial distribution of the constant-size default model (defaultEta)
    std::vector<unsigned char> key_nbpos;  // [K] key.nb() > 0
    std::vector<Chunk> chunks;
    int max_chunks_per_contig = 1;
    int user_rows_per_chunk = 0;
    StatsLayout lay;                       // sorted permutations, slabs, ranges, teams and sizes of the statistics (cut_stats_layout)
    GammaPieces gp;
    StatsLayout cut_stats_layout() const;
    void build_gamma_pieces();
    // ---- parameters -------------------------------------------------------------------------------------------
    double theta = NAN, rho = NAN, alpha = 1.0;
    bool have_raw = false, dirty = true, params_fresh = false;
    // a setter: the prepared tables go; results_stale: so do the last E-step's vectors; model_setter: a manager with a model leaves the raw path
    void params_changed(bool model_setter, bool results_stale = true) { params_fresh = false; ss_range_refused = false; dirty = dirty || results_stale; have_raw = have_raw && !(model_setter && have_model); }
    std::vector<double> pi, T, E;          // [M], [M*M], [K*M]
    smcpp_host::ModelParams model;         // a, s (for set_params); the distinguished model of a two-population manager
    smcpp_host::ModelParams model_p1, model_p2;          // two populations: per-population pieces (set_params_twopop)
    std::vector<double> model_da1, model_da2;            // their derivative seeds [K x nder]
    double split = 0.0;
    std::vector<double> model_da;          // [Kp x nder] derivative seeds of a
    int nder = 0;
    std::vector<double> dpi, dT, dE;       // Jacobians [size x nder] of pi, T, E w.r.t. the seeds
    std::vector<double> emission, demission;   // InferenceManager::emission [M x cols] (+ Jacobian), model path only
    bool have_model = false;
    bool save_gamma = false, gamma_valid = false, estep_done = false;
    // ---- device -----------------------------------------------------------------------------------------------
    int device = 0;
    hipStream_t stream3 = nullptr;         // third branch of the statistics (log-likelihood or per-key gamma sums)
    hipStream_t stream = nullptr, stream2 = nullptr;   // stream2: backward chain when it may overlap the forward one
    hipStream_t stream_hi = nullptr;       // per-row gammas beside the statistics
    // Event slots: every record and wait names what it orders
    enum Ev {
        EV_ESTEP, EV_FIRST_PASS,           // E-step start; in front of the first chain launch (eigen-free pre-pass or scan chains)
        EV_PRE_FWD_END, EV_PRE_BWD_START, EV_PRE_BWD_END,           // eigen-free pre-pass: the forward and backward chains' intervals
        EV_CHAINS_START, EV_BWD_START, EV_FWD_END, EV_CHAIN_SYNC,   // dense chains: intervals, hand-over between their two streams
        EV_CHAINS_END, EV_STATS_FORK,      // behind the last pass (the statistics' fork on the scan chains); fork on the dense ones
        EV_ARENA,                          // the parameter arena copied on the second stream has landed
        EV_LOGLIK_DONE, EV_RANK2_DONE, EV_S1_SCALARS, EV_GSUM_FORK, EV_GSUM_DONE, EV_SPAN1_DONE, EV_SIDE_DONE,   // statistics branches
        EV_GAMMA_FORK, EV_GAMMA_DONE,      // per-row gammas beside the statistics
        EV_STATS_DONE, EV_COUNT            // end of the E-step's queue
    };
    hipEvent_t ev[EV_COUNT];
    int dual_stream = 1;
    void read_dual_stream() { dual_stream = opt().i(smcpp_opt::O_DUAL_STREAM, 1); }      // (build_device; a host-only manager's hook)
    bool chains_dual = false;
    DevBuf<RowInfo> d_rowinfo;
    DevBuf<int2> d_rowdesc;
    DevBuf<long long> d_dbg;
    DevBuf<float> d_qTf;
    DevBuf<double> d_qTdT, d_qPinvT, d_qPT, d_qPrm, d_qPinvrm;   // quarter-interleaved operands of the big-M chains
    int cu_count = 0;                      // compute units of the device (build_device), the one device fact the plan uses
    ChainPlan plan;                        // of this manager and chunking (make_chunks)
    ChainPass chain_pass;                  // of the last E-step on the scan chains (ss_launch_initial)
    ChainPlan resolve_chain_plan(int compute_units, const ChainPlan *previous) const;
    ChainPass resolve_chain_pass() const;
    void cut_chunks(const ChainPlan &p);
    // ---- chains on the semiseparable structure of T (chains_ss.hpp; chain family 5) -----------------------------------------
    std::unique_ptr<smcpp_host::OnePopPrep> prep1;   // one-population cold preparation (caches per-key tables)
    std::vector<double> prep1_hs;
    // device cold preparation (prep_dev.hpp): the emission table of the current parameters lives on the device only and the host
    // vectors E / dE / emission / Eg are stale until sync_host_E() fetches them (getters, non-lean E-steps)
    std::unique_ptr<DevPrep> dprep;
    bool E_on_dev = false, force_host_prep = false;
    ParamPlan param_plan; EstepRoute estep_route;         // of the last prepare_params() / set_raw; of the last E-step (smcpp_describe: "parameters")
    ParamPlan resolve_param_plan() const;
    EstepRoute resolve_estep_route(bool structured_T, bool underflow = false) const;     // underflow: why the scan chains are refused (ss_underflow)
    void dev_prepare(const std::vector<int> &pk, int Kp_);     // (the prepared key list: global or this rank's)
    void sync_host_E();
    void fetch_prepared_table(std::vector<double> &E_out, std::vector<double> &dE_out, bool whole);     // the device's table -> host (whole: + emission, Eg / dEg)
    void scatter_prepared_table(std::vector<double> &Ep, std::vector<double> &dEp, std::vector<double> &E_out, std::vector<double> &dE_out, bool keep_global);
    // Q and its gradient on the device (prep_dev.hpp: k_q_reduce): the O(M) generators of the transition matrix with their
    // derivative planes (host, prep.hpp: transition_generators_jac; dT is expanded on the host only when its getter asks)
    smcpp_host::TransitionGenJac tgen;
    bool tgen_valid = false, dT_valid = true;
    // (round 6) the device-prepared model path keeps the O(M) generators of T and expands the M x M matrix only when somebody reads it
    // (ensure_T): the scan chains take their operator from the generators (ss_generators_from_tgen), so the expansion - 51 us at
    // M = 256 - and the entry-by-entry structure check of the expanded matrix - 58 us - leave the critical path in front of the chains;
    // host_prep_and_upload expands it for the statistics while the chains run
    bool T_lazy = false;
    // ... and the scan chains keep taking their operator from the generators for as long as these parameters stand, also after the
    // matrix was expanded (by the statistics of the first E-step, or by a getter): an E-step repeated with the same parameters runs
    // on the same generators, bit for bit, whoever read T in between (the generators extracted back from the expanded matrix differ
    // from them in the last bits)
    bool T_from_gen = false;
    // host preparations, set_raw.  T_from_gen is left standing: tgen_valid == false disarms its one reader (ss_extract_generators)
    void params_on_host_route() { E_on_dev = false; tgen_valid = false; dT_valid = true; T_lazy = false; }
    smcpp_host::TransitionGenerators<double> tgen_g;
    void ensure_T() { if (T_lazy) { T = smcpp_host::transition_expand<double>(tgen_g); T_lazy = false; } }
    struct QDev {
        DevBuf<double> d_stats, d_out;
        DevBuf<int> d_keynb;
        PinnedArena stage;
        char *d_in = nullptr;
        size_t in_cap = 0;
        double *h_out = nullptr;
        size_t h_out_cap = 0;
        bool stats_ready = false;
        int Kq = 0;
        ~QDev() { if (d_in) (void)hipFree(d_in); if (h_out) (void)hipHostFree(h_out); }
    };
    std::unique_ptr<QDev> qdev;
    bool q_device(double val[4], double *jac);
    enum { Q_ROUTE_NONE = 0, Q_ROUTE_DEVICE, Q_ROUTE_HOST };
    int q_route = Q_ROUTE_NONE;            // who evaluated the last smcpp_q (smcpp_describe: "q_route")
    void ensure_dT();
    // hybrid rows cost about SS_HYB_COST scan positions each, which is what the chunk list is balanced on
    static constexpr int SS_HYB_COST = 8;
    static long long ss_row_cost(const ChainPlan &p, int span) { return (p.hybrid && span > p.hyb_th) ? SS_HYB_COST : span; }
    // Power jumps of the scan chains (chains_ss.hpp): in the history passes, every P scan steps inside a row of ONE key become one
    // mat-vec by the P-th power of that key's operator.  resolve_chain_plan() decides key and power once per manager.
    // What it charges a jump when it asks whether jumps remove 5 % of the chain work: 3 permlane swaps + 64 fused
    // multiply-adds + 4 adds against the 25 (forward) / 38 (backward) instructions of a light-pass position.  Instruction counts,
    // not a measurement; nothing else reads it (chunks are cut by positions).
    static constexpr int SS_JUMP_COST = 3;
    bool ss_jump_on() const { return plan.jump_P != 0 && plan.scan && !plan.hybrid && NPL == 1; }
    // cost of a row in scan positions with the jumps taken: the first position, the jumps, the scan steps that remain
    static long long ss_jump_cost(int span, int P) { const long long r = span - 1; return 1 + (r / P) * SS_JUMP_COST + r % P; }
    // (the chunk lists stay cut by POSITIONS, jumps or not: seams, halos and every count of the plan are where they were - what
    // tests/test_gpu_seams.py places its features on)
    DevBuf<float> d_jtab_f;                // [2][64][64] off-diagonal part of the power table and its transpose, rebuilt on every E-step
    DevBuf<double> d_jdiag;                // [64] its diagonal
    // LDS the hybrid rows' eigenvector tables take (+ one scratch vector per wavefront)
    static size_t ss_tab_bytes(const ChainPlan &p, int Mp) { return p.hybrid ? ((size_t)p.nk_lds * (p.dirsplit() ? 2 : 4) * Mp * (Mp + 1) + 8 * 64) * sizeof(double) : 0; }
    int ss_max_span = 0;                   // the longest row (build_layout)
    // what run_chains_ss learns (state, not plan)
    int ss_launched = 0, last_ss_passes = 0;
    bool ss_need_cert_pass = false;     // this input's last working pass rewrites end vectors within tolerance: launch the all-skip pass up front
    // opt-in warm start of the scan chains (smcpp_set_warm_start): the first pass of an E-step starts every chunk from the boundary
    // vector the PREVIOUS converged E-step left (parity ss_warm_parity of the end-vector arrays) instead of pi / the uniform
    // vector, and one light pass fewer runs; pass indices then start at ChainPass::pass0 (1 or 2: the parity the first pass reads)
    bool ss_warm_valid = false;
    int ss_warm_parity = 0;
    std::vector<int> ss_slot_of_key;       // frequency rank of every key (slot 0 = most rows)
    DevBuf<int2> d_rowdesc_ss;             // [rows, padded] {key slot, span}
    // rows of binned data longer than 64 positions, cut into pieces at construction (build()): the caller's row counts, the pieces'
    // rows (what every kernel sees) and piece -> caller's row, per contig (1-based rows; entry 0 = row 0)
    bool split_spans = false;
    std::vector<int> user_Ls;
    std::vector<std::vector<int>> split_store, piece_row;
    std::vector<const int *> split_ptr;
    std::vector<DevBuf<int>> d_piece_first;       // per contig: first piece of every caller's row ([Lu + 2]; k_gamma_merge)
    DevBuf<double> d_gamma_user;                  // the caller's rows of ONE contig, pieces added up: [Lu + 1][Mp]
    const double *merged_gamma(int c);            // (device pointer; row 0 unset)
    // posterior products (posterior_dev.hpp, smcpp_posterior_*): prefix positions of the CALLER's rows per contig ([Lu + 1], entry 0 =
    // 0; built in build(), uploaded on first use) and the device side of the outputs
    std::vector<std::vector<long long>> user_prefix;
    std::vector<DevBuf<long long>> d_user_prefix;
    DevBuf<double> d_post_out, d_post_colsum, d_post_mean, d_post_w;
    DevBuf<int> d_post_arg, d_post_q;
    struct PostSource { const double *rows, *g0; int L; };
    PostSource post_source(int c);                // (after the argument checks: may launch k_gamma_merge)
    void post_columns(int c, long long start, long long stop, long long step, bool normalize, bool f32, void *out, double *colsum);
    // what the product calls share (engine_products.hpp): the generators of the last E-step's T on the device (constants of the
    // E-step, uploaded by every walking call), the host-side set-up of a walk over the stored vectors
    DevBuf<double> d_walk_gen;
    SsArgs walk_generators();                     // ss_gen -> d_walk_gen on `stream`; a fresh SsArgs with M, Mp and the generators set
    WalkRows walk_rows(int c);                    // the stored vectors and the row table a walk over contig c reads
    int longest_row(int c);                       // the longest engine row of contig c
    long long walk_slots() const;                 // wavefront slots of a persistent walk
    const long long *user_prefix_dev(int c);      // user_prefix[c] on the device, uploaded on first use
    // posterior transition products (posterior_trans_dev.hpp, smcpp_posterior_transition*): the wavefronts' scratch (parked addends,
    // checkpoints of long rows), the products per engine row and per selected caller's row
    DevBuf<double> d_pt_ckpt, d_pt_eng, d_pt_sel;
    DevBuf<float> d_pt_park;
    const int *piece_first_dev(int c);            // first piece of every caller's row of contig c on the device; nullptr: no row is cut
    void post_transitions_check();                // throws unless the stored vectors and a structured T are there
    const double *post_transitions(int c, long long start, long long step, long long ncols);   // -> [3][ncols] on the device
    // posterior paths (posterior_paths_dev.hpp, smcpp_posterior_sample_*): the transposed dense T, the wavefronts' scratch (parked
    // forward vectors of a block, checkpoints of long rows), state / up / down per path and engine row, per selected caller's row,
    // and the states per path and position of a window
    DevBuf<double> d_pp_TT, d_pp_ckpt;
    DevBuf<float> d_pp_park;
    DevBuf<int> d_pp_eng, d_pp_sel, d_pp_pos;
    int pp_batch = 0;                             // paths per wavefront of the last call (smcpp_describe)
    long long pp_batches = 0;                     // batches of the last call
    int pp_waves = 0, pt_waves = 0;               // wavefronts launched by the last path / transition call (smcpp_describe)
    struct PostPaths { const int *rows, *pos; };
    // rows: [3][npaths][ncols] of the selection (ncols > 0), pos: [npaths][pos1 - pos0] (pos1 > pos0), on the device, on `stream`
    PostPaths post_paths(int c, unsigned long long seed, long long path0, long long npaths, long long start, long long step,
                         long long ncols, long long pos0, long long pos1);
    // simulation (simulate_dev.hpp, smcpp_simulate): the padded dense T, the alphabet's emission table by state, the per-state
    // vectors (log s | stay-loud weight | pi), the contig lengths, the resume triples and the per-replicate outputs
    DevBuf<double> d_sim_T, d_sim_EA, d_sim_vec;
    DevBuf<long long> d_sim_len, d_sim_rin, d_sim_rout, d_sim_nev, d_sim_pos;
    DevBuf<int> d_sim_x0, d_sim_state, d_sim_key;
    int sim_waves = 0;                            // wavefronts of the last simulate call (smcpp_describe)
    long long sim_units = 0, sim_events = 0;      // its (contig, replicate) pairs and the loud positions it wrote
    // posterior positions (posterior_pos_dev.hpp, smcpp_posterior_positions / _position_summary / _windows_exact): the item table of
    // the last call (engine rows to walk, positions whose marginal is stored), the wavefronts' scratch, the segment sums of the
    // rows a window boundary cuts
    std::vector<PqItem> pq_items;
    std::vector<long long> pq_start;              // segments: the position in front of every item
    DevBuf<PqItem> d_pq_items;
    DevBuf<long long> d_pq_start;
    DevBuf<float> d_pq_park;
    DevBuf<double> d_pq_ckpt, d_pq_seg, d_pq_colsum;
    int pq_waves = 0;                             // wavefronts of the last position call (smcpp_describe)
    long long pq_walked = 0;                      // engine rows it walked
    int pq_smax = 1;                              // the longest of them
    long long pq_nseg = 0;
    void post_positions_grid(int c, long long pos0, long long pos1, long long step);     // -> pq_items (host)
    void post_positions_segments(int c, long long W);                                    // -> pq_items, pq_start, pq_nseg (host)
    void post_positions_scratch_check(size_t extra_bytes);                               // throws beyond the 1 GiB cap
    const double *post_colsum(int c, const PostSource &src, DevBuf<double> &dst);        // [Lu + 1] column sums on the device, in dst
    void post_positions_launch(int c, int kind, PqArgs &pa);
    // log-likelihood track (loglik_track_dev.hpp, smcpp_loglik_rows / _positions / _windows): buffers of its own - the posterior
    // products' are neither read nor written.  The position prefix of the ENGINE's rows per contig (where rows are cut; otherwise the
    // caller's prefix serves), the prefix of log c over one contig's engine rows, the item table of the last call, its outputs
    std::vector<DevBuf<long long>> d_ll_epos;
    std::vector<LlItem> ll_items;
    DevBuf<LlItem> d_ll_items;
    DevBuf<double> d_ll_part, d_ll_pre, d_ll_out, d_ll_bnd, d_ll_ratio;
    std::vector<double> ll_ratio_h;
    long long ll_nslots = 0;                      // slots the items of the last table write
    int ll_waves = 0;                             // wavefronts of the last walk (smcpp_describe)
    long long ll_nitems = 0;                      // its items
    double ll_worst = 0.0;                        // the worst |A_span / log c_r - 1| of the last call
    const long long *ll_epos_dev(int c);          // EP [Le + 1] on the device
    const double *ll_prefix(int c);               // pre [Le + 1] on the device, on `stream`
    void ll_table(int c, long long pos0, long long pos1, long long step, bool windows);   // -> ll_items, ll_nslots (host)
    void walk_item_table(int c, long long pos0, long long pos1, long long step, bool windows, std::vector<LlItem> &items,
                         long long &nslots) const;                                        // the builder behind it: -> the caller's table
    void ll_walk(int c, long long step, double *slots);                                   // k_ll_walk over ll_items (not empty)
    // score track (score_track_dev.hpp, smcpp_score_rows / _windows): buffers of its own - the posterior products' and the loglik
    // track's are neither read nor written.  The tables G_pi | dT | G_E of the last E-step's parameters (built from the host Jacobians
    // on the first call behind an E-step), the checkpoints of long rows, the parts per engine row, per selected caller's row, the
    // windows (the generators travel in d_walk_gen, as for every walking call)
    DevBuf<double> d_sc_tab, d_sc_ckpt, d_sc_eng, d_sc_sel, d_sc_out;
    bool sc_tab_valid = false;                    // d_sc_tab belongs to the last E-step (cleared by estep())
    int sc_waves = 0;                             // wavefronts of the last score call (smcpp_describe)
    long long sc_items = 0;                       // engine rows it walked
    int score_check(int c);                       // throws unless a score call can run on contig c; -> checkpoint vectors per wavefront
    void score_tables();                          // -> d_sc_tab (keeps E_on_dev: a later smcpp_q stays on its device route)
    const double *score_rows(int c, long long start, long long step, long long ncols, int parts, int nck);   // -> device, on `stream`
    // ... in its VECTOR form (score_vec_dev.hpp; SMCPP_SCORE_FORM=vectors, read at every call): G_pi | the four coefficient planes of
    // the transition Jacobian | G_E, each 64 NPL wide, from the generator planes `tgen` - the dense dT is not expanded
    DevBuf<double> d_sv_tab;
    DevBuf<float> d_sv_park;
    bool sv_tab_valid = false;                    // d_sv_tab belongs to the last E-step (cleared where sc_tab_valid is)
    bool sc_vectors = false;                      // the form of the last score call (smcpp_describe)
    bool score_form_vectors() const;              // what SMCPP_SCORE_FORM asks for now (throws on a value it does not know)
    void score_tables_vec();                      // -> d_sv_tab (keeps E_on_dev as score_tables does)
    void score_rows_vec(int c, int nck);          // k_score_rows_vec -> d_sc_eng, on `stream`
    void score_rows_matrix(int c, int nck);       // k_score_rows -> d_sc_eng, on `stream`
    // ... and its EXACT windows (score_seg_dev.hpp, smcpp_score_windows_exact; the vectors form only): the table of the engine rows a
    // window boundary cuts - the loglik track's builder, a table, slots and outputs of its own (ll_items and the d_ll_* buffers are
    // neither read nor written) -, the parts per segment of a cut row, the windows.  The parked blocks and checkpoints are the row
    // walk's (d_sv_park, d_sc_ckpt: the segment walk runs behind it on `stream`)
    std::vector<LlItem> sx_items;
    long long sx_nslots = 0;                      // the segments of the last table: nq + 1 per item
    DevBuf<LlItem> d_sx_items;
    DevBuf<double> d_sx_seg, d_sx_out;
    long long sx_nitems = 0, sx_nseg = 0;         // the items and segments of the last exact call (smcpp_describe)
    int sx_waves = 0;                             // the wavefronts of its segment walk (0: it was not launched)
    void score_segments_vec(int c, int nck, long long W, long long nw);   // k_score_segments_vec over sx_items (not empty) -> d_sx_seg
    bool ss_generators_only();            // the generators of T into ss_gen / ss_c0 (no underflow bound: the walks rescale every step)
    DevBuf<float> d_gpark;                 // k_gamma_rows_scan: [wavefronts][max span][64 NPL] parked forward vectors
    SsArgs ss_args;
    std::vector<Chunk> chunks_b;           // backward chunks of the scan chains (more and shorter than the forward ones)
    std::vector<int> ss_tasks;             // (direction << 30 | chunk) per wavefront of a k_chain_ss launch
    DevBuf<Chunk> d_chunks_b;
    DevBuf<int> d_tasks;
    void update_pi_default();
    bool debug = false;                    // InferenceManager::debug (_smcpp.pxd:53): declared by the reference, read by nothing
    void upload_chunk_state();
    bool ss_extract_generators();          // generators of T (verified entry by entry) into ss_gen; false: T has no such structure,
                                           // or (ss_underflow) an emission entry of a host table is too small for `span` scan steps
    bool ss_underflow = false;
    // the scan chains ran on these parameters and a row's evidence left the range of their float intermediates (kernels.hpp:
    // LoglikArgs::range_flag, read by estep()): until the parameters change, ss_extract_generators refuses them like a bound
    bool ss_range_refused = false;
    // the last E-step ran twice: the scan chains' attempt on a device-prepared table was abandoned (DevPrep flag 2) and the E-step
    // redone on the dense kernels (smcpp_describe: "estep_redone", "estep_redone_why")
    bool estep_redone = false;
    const char *estep_redone_why = "";
    std::vector<double> ss_gen;            // [10][MS]: f_dc f_g f_cg f_b f_a f_d b_dc b_g b_b b_a
    double ss_c0 = 0.0;
    void ss_launch_initial();
    void ss_launch_passes(int upto);
    bool run_chains_ss();                  // false: not converged on a device table that DevPrep flag 2 names (estep redoes it)
    int hot_eig = -1, hot_eig2 = -1;
    // eigen-free pre-pass (chains2.hpp: k_group_powers, POWER instantiations): pass 0 runs on group powers while the host
    // solves the eigenproblems; only for short, few spans (binned data) and chunks short enough that pass 1 re-runs them whole
    // (ChainPlan::power_ok)
    bool prepass_launched = false;
    PinnedArena pre_stage;                 // static operands of the pre-pass (pi, T, emission table): own pinned mirror
    char *d_pre = nullptr;
    size_t pre_cap = 0;
    bool static_packed = false;
    float pre_f_ms = 0.f, pre_b_ms = 0.f;
    DevBuf<float> d_Bf;                    // [Ke][4][Mp][Mp] binary powers A^2..A^16 per eigen key (forward operand)
    DevBuf<double> d_Bb;                   // [Ke][4][Mp][Mp] their transposes (backward operand)
    // pre-pass of the streamed-operand chains (64 < M <= 256): device-built layouts of T and of the powers A .. A^16
    DevBuf<double> d_W, d_pre_qTdT;        // [Ke][nbits][Mp][Mp] row-major powers (fp64) / [KQ][Mp][4]
    DevBuf<float> d_qBf, d_qBb, d_pre_qTf; // [Ke][nbits][KQ][Mp][4] float streaming layouts / [KQ][Mp][4]
    BigArgs pre_bargs;
    std::vector<std::unique_ptr<smcpp_host::EigTeam>> eig_teams;    // team-parallel eigensolver (M >= 128), one team per eigen key
    DevBuf<Chunk> d_chunks;
    DevBuf<int> d_g_span, d_g_eig, d_e_kid, d_contig_L, d_changed_f, d_changed_b, d_argmax;
    DevBuf<long long> d_contig_base;
    DevBuf<float> d_pi_f, d_Tf, d_alpha, d_ends_f, d_used_f;
    DevBuf<double> d_E, d_dpow, d_PinvT, d_PT, d_TdT, d_Td, d_Prm, d_Pinvrm, d_dsc, d_dun, d_g_scale,
        d_g_logscale, d_beta, d_cnorm, d_logc, d_ends_b, d_used_b, d_llpart, d_loglik, d_w1, d_gpart, d_Xs, d_Ys,
        d_red_1, d_red_g, d_Z, d_Y, d_xisum, d_gsum, d_gamma0, d_gamma_rows, d_Sq;
    // sized from the plan of an E-step, by size_stats_buffers() alone (d_Fall: [n_contigs Ke][smax][Mp][Mp] scratch of the span fold)
    DevBuf<double> d_part_1, d_gpart_fk, d_part_e, d_red_e, d_part_ek, d_red_ek, d_Zpart, d_Fall;
    void size_stats_buffers(const StatsPlan &p);
    // opt-in warm start: chunk-boundary vectors of the previous converged E-step (see smcpp_set_warm_start)
    bool warm_start = false, warm_valid = false;
    DevBuf<float> d_warm_f;
    DevBuf<double> d_warm_b;
    DevBuf<unsigned char> d_present;       // device copies used by k_pack_stats
    DevBuf<int> d_g2l;
    bool pack_tables_ready = false;
    std::vector<double> hs_PinvT, hs_PT, hs_Prm, hs_Pinvrm, hs_dsc, hs_dun, hs_dpow, hs_gsc, hs_gls, hs_TdT, hs_Td, hs_Ep;
    std::vector<float> hs_pi_f, hs_Tf;      // host staging of the per-E-step parameter arrays (see host_prep_and_upload)
    PinnedArena stage;
    char *d_param = nullptr;      // device side of the per-E-step parameter arena
    int *h_flags = nullptr;       // pinned: per-pass "something re-ran" flags of both chains, read back every round
    // scan-chain E-steps: the chain kernels write their flags and the log-likelihood kernel its result STRAIGHT into pinned host
    // memory (device views below) and a one-thread kernel at the end of the queue raises h_done; the host polls that word - no
    // small copies or fills on the stream, no blocking wait (together ~30 us of a 1.4 ms eval)
    int *d_flags_view = nullptr;  // device address of h_flags
    double *d_ll_view = nullptr;  // device address of h_ll
    int *h_done = nullptr, *d_done_view = nullptr;
    struct RcclDirect *rccl = nullptr;       // the E-step's exchange issued from here, on `stream` (smcpp_rccl_* below); owned
    int done_epoch = 0;
    DevBuf<unsigned> d_fin_ctr;          // blocks of the finalisation launches that raise h_done themselves (k_fin_both)
    unsigned fin_target = 0;
    bool timing_pending = false;         // the event intervals of the last E-step are read when somebody asks (resolve_timing)
    double t_host01 = 0, t_host12 = 0;
    void resolve_timing();
    bool done_covers_stats = false;
    bool wait_done(int epoch);
    double *h_ll = nullptr;       // pinned: per-contig log-likelihoods
    int h_flags_cap = 0, h_ll_cap = 0;
    size_t param_cap = 0;
    int last_fwd_passes = 0, last_bwd_passes = 0;
    float eps_f = 2e-6f;
    double eps_b = 1e-6;   // relative; beta only enters products with the float alpha (noise floor 2e-6), see DESIGN.md §3
    // ---- results (host) ---------------------------------------------------------------------------------------
    std::vector<double> loglik, h_xisum, h_gsum, h_gamma0;
    bool stats_on_host = false;
    double timing[9] = {0};
    double host_timing[4] = {0};   // [cold preparation A6-A10, eigensystems, layouts + staging, whole host phase] of the last E-step, ms
    // multi-GPU
    std::vector<int> gkeys;                // global key list [Kg][keylen]
    std::vector<int> local_to_global;
    bool have_global = false;
    std::vector<double> g_stats;           // reduced [1 + M + M*M + Kg*M]
    bool have_reduced = false;
    // emission vectors (and Jacobians) of EVERY global key, so that Q on the all-reduced statistics also covers keys
    // that only other ranks' contigs hold; rows of keys nobody supplied (set_raw) are NaN
    std::vector<double> Eg, dEg;
    std::vector<int> raw_keys;             // what the last set_raw handed over: [Kr][keylen], raw_E [Kr][M]
    std::vector<double> raw_E;
    void global_emissions();

    ~smcpp_im() {
        if (stream) {
            for (auto &e : ev) (void)hipEventDestroy(e);
            (void)hipStreamDestroy(stream);
            if (stream2) (void)hipStreamDestroy(stream2);
            if (stream3) (void)hipStreamDestroy(stream3);
            if (stream_hi) (void)hipStreamDestroy(stream_hi);
        }
        if (d_param) (void)hipFree(d_param);
        if (d_pre) (void)hipFree(d_pre);
        if (h_flags) (void)hipHostFree(h_flags);
        if (h_ll) (void)hipHostFree(h_ll);
        if (h_done) (void)hipHostFree(h_done);
    }

    void build(int npop_, const int *nn, const int *nna, int n_contigs_, const int *Ls_, const int *const *obs,
               int n_hs, const double *hs_, double pol, int dev);
    // its two halves: the host layout (keys, rows, groups, the cut of long rows; no device call) and the device part
    void build_layout(int npop_, const int *nn, const int *nna, int n_contigs_, const int *Ls_, const int *const *obs,
                      int n_hs, const double *hs_, double pol);
    void build_device(int dev);
    // the plan of this chunking (user_rows_per_chunk) and its chunk lists; a re-plan (smcpp_set_chunking) keeps what is per manager
    void make_chunks() { plan = resolve_chain_plan(cu_count, plan.resolved ? &plan : nullptr); cut_chunks(plan); }
    void alloc_device();
    void host_prep_and_upload();
    void stage_static_and_prepass();
    void setup_power();
    ChainArgs chain_args(const ChainPass &cp);
    void run_chains();
    void run_stats();            // = enqueue_stats() unless run_chains() already queued them, + finish_stats()
    // signal_epoch != 0: nothing follows on the main stream, and the statistics may raise the completion word with this epoch
    // themselves; returns whether they do
    bool enqueue_stats(int signal_epoch = 0);
    void finish_stats();
    bool stats_enqueued = false;
    StatsPlan stats_plan;        // of the last enqueue_stats()
    StatsPlan resolve_stats_plan(bool generators) const;
    // save_gamma's long rows at 64 < M <= 256 may take the eigen-power pieces, if generators of T exist (the resolver's `generators`)
    bool gamma_pieces_fit() const {
        return save_gamma && lay.n_e_rows > 0 && !estep_route.eigfree && NT > 4 && Mp <= 256 && !opt().off(smcpp_opt::O_GAMMA_PIECES) &&
               (double)lay.pieces * Mp * 20.0 < 96e9;
    }
    // (enqueue_stats' helpers and branch launchers)
    hipStream_t plan_stream(StatsPlan::Stream x) const {
        return x == StatsPlan::SECOND ? stream2 : x == StatsPlan::THIRD ? stream3 : x == StatsPlan::HIGH ? stream_hi : stream;
    }
    // what is queued on `from` so far precedes what is queued on `to` from now on
    void hand_over(Ev e, hipStream_t from, hipStream_t to) { HIPCHK(hipEventRecord(ev[e], from)); HIPCHK(hipStreamWaitEvent(to, ev[e], 0)); }
    void fork_from_chains(hipStream_t x);
    S1Args s1_args(bool span_gt1);
    AccArgs acc_args(const HostDev<Slab> &sl, const int *perm, const int2 *permk, double *part, double *gpart);
    void launch_span_gt1_rank(const StatsPlan &p), launch_span1_branch(const StatsPlan &p), launch_gamma_rows(const StatsPlan &p);
    void launch_span_gt1_branch(const StatsPlan &p, FinArgs &fa);
    void estep(bool redo = false);         // redo: estep()'s own second entry (the redo above)
    void fetch_stats();
    void prepare_params();
};

// ---------------------------------------------------------------------------------------------------------------
// construction
// ---------------------------------------------------------------------------------------------------------------
void smcpp_im::build(int npop_, const int *nn, const int *nna, int n_contigs_, const int *Ls_,
                     const int *const *obs, int n_hs, const double *hs_, double pol, int dev) {
    build_layout(npop_, nn, nna, n_contigs_, Ls_, obs, n_hs, hs_, pol);
    build_device(dev);
}

void smcpp_im::build_layout(int npop_, const int *nn, const int *nna, int n_contigs_, const int *Ls_,
                            const int *const *obs, int n_hs, const double *hs_, double pol) {
    npop = npop_;
    keylen = 3 * npop;
    for (int p = 0; p < npop; ++p) { n[p] = nn[p]; na[p] = nna[p]; }
    polarization_error = pol;
    if (n_contigs_ <= 0) throw std::runtime_error("Observations list is empty");
    if (n_hs < 2) throw std::runtime_error("need at least two hidden state boundaries");
    hs.assign(hs_, hs_ + n_hs);
    for (int i = 1; i < n_hs; ++i)
        if (!(hs[i] >= hs[i - 1])) throw std::runtime_error("Hidden states must be in ascending order");
    M = n_hs - 1;
    Mp = (M + 15) / 16 * 16;
    // states per lane of the one-wavefront-per-chunk kernels: 1 .. 4 up to M = 256; 256 < M <= 512 (round 5): eight - the scan chains
    // and the eigen-free statistics only (binned data, a transition matrix with the reference's structure, no save_gamma: what
    // `smc++ estimate` runs); the dense fallback kernels and the eigensystem statistics stop at 256
    // (round 6) 512 < M <= 1024: sixteen states per lane, the same restriction
    NPL = M > 512 ? 16 : M > 256 ? 8 : (M + 63) / 64;
    NT = Mp / 16;
    if (M > 1024) throw std::runtime_error("M > 1024 hidden states is not supported by this build");
    n_contigs = n_contigs_;
    Ls.assign(Ls_, Ls_ + n_contigs);
    user_Ls = Ls;
    // (round 6) Long rows of BINNED data cut into pieces of at most 64 positions.  A row of span s with key k is s identical positions;
    // the rows (s1, k), (s2, k) with s1 + s2 = s are the same positions: the same likelihood, the same xi sums and gamma sums, and
    // the row's posterior (hmm.cpp:113-121: the sum over its positions, normalised to s) is the sum of the pieces' posteriors.  The
    // eigen-free statistics walk a span in at most 64 steps (k_span_scan) and are all that exists beyond 256 states; up to 256 the
    // alternative for such rows is an eigensolve of every key's M x M operator on the host per E-step.  So for M > 64 the pieces are
    // what every kernel sees; the getters that report per row (gamma, its argmax, the column count) add the pieces up again.
    // Only where the pieces stay few: un-binned data (spans of 10^4 - 10^5 base pairs) keep their rows and the eigen-power steps.
    {
        const int ncol_ = 1 + keylen;
        long long rows = 0, pieces = 0;
        int maxspan = 0;
        user_prefix.assign(n_contigs, std::vector<long long>());
        for (int c = 0; c < n_contigs; ++c) {
            std::vector<long long> &pp = user_prefix[c];
            pp.assign((size_t)std::max(Ls[c], 0) + 1, 0);
            for (int i = 0; i < Ls[c]; ++i) {
                const int sp = obs[c][(size_t)i * ncol_];
                if (sp <= 0) throw std::runtime_error("data are malformed: span <= 0");
                rows++; pieces += (sp + 63) / 64; maxspan = std::max(maxspan, sp);
                pp[(size_t)i + 1] = pp[i] + sp;
            }
        }
        const bool want = M > 64 && !opt().off(smcpp_opt::O_SPLIT_SPANS);      // (M <= 64: the one-state-per-lane chains have no un-floored store)
        // (beyond 256 states there is no other path: un-binned rows are cut as well - the chains then walk every position, which is
        // what a row costs there anyway - as long as the pieces' alpha / beta rows fit a third of a 288 GB device)
        const bool few = pieces <= 2 * rows + 1024;
        const bool must = (M > 256 || opt().i(smcpp_opt::O_SPLIT_SPANS, 1) == 2) && (double)pieces * (double)Mp * 12.0 < 96e9;   // (=2: test switch)
        split_spans = want && maxspan > 64 && (few || must);
        if (split_spans) {
            split_store.assign(n_contigs, std::vector<int>());
            split_ptr.assign(n_contigs, nullptr);
            piece_row.assign(n_contigs, std::vector<int>());
            for (int c = 0; c < n_contigs; ++c) {
                std::vector<int> &so = split_store[c];
                std::vector<int> &pr = piece_row[c];
                pr.push_back(0);                              // (internal row 0 = the caller's row 0: the initial distribution)
                for (int i = 0; i < user_Ls[c]; ++i) {
                    const int *r = obs[c] + (size_t)i * ncol_;
                    for (int left = r[0]; left > 0; left -= 64) {
                        so.push_back(std::min(left, 64));
                        so.insert(so.end(), r + 1, r + ncol_);
                        pr.push_back(i + 1);
                    }
                }
                Ls[c] = (int)(so.size() / ncol_);
                split_ptr[c] = so.data();
            }
            obs = split_ptr.data();
        }
    }
    contig_base.resize(n_contigs);
    total_rows = 0;
    for (int c = 0; c < n_contigs; ++c) {
        if (Ls[c] <= 0) throw std::runtime_error("empty contig");
        contig_base[c] = total_rows;
        total_rows += (long long)Ls[c] + 1;
    }
    const int ncol = 1 + keylen;
    // key dictionary (populate_emission_probs, inference_manager.cpp:190-211): distinct keys, lexicographic
    std::map<std::vector<int>, int> kmap;
    for (int c = 0; c < n_contigs; ++c) {
        const int *ob = obs[c];
        std::vector<int> prev;
        for (int i = 0; i < Ls[c]; ++i) {
            const int *r = ob + (size_t)i * ncol;
            if (r[0] <= 0) throw std::runtime_error("data are malformed: span <= 0");
            if (!prev.empty() && std::equal(prev.begin(), prev.end(), r + 1)) continue;
            prev.assign(r + 1, r + ncol);
            kmap.emplace(prev, 0);
        }
    }
    K = (int)kmap.size();
    keys.clear();
    {
        int id = 0;
        for (auto &kv : kmap) { kv.second = id++; keys.insert(keys.end(), kv.first.begin(), kv.first.end()); }
    }
    key_nbpos.assign(K, 0);
    for (int k = 0; k < K; ++k) {
        int nb = 0;
        for (int p = 0; p < npop; ++p) nb += keys[(size_t)k * keylen + 3 * p + 2];
        key_nbpos[k] = nb > 0;
    }
    // rows -> (kid, span); fill_targets (inference_manager.cpp:232-254): distinct (span > 1, key) pairs
    rowinfo.assign((size_t)total_rows, RowInfo{0, -1});
    std::vector<int> span_of((size_t)total_rows, 1);
    present.assign((size_t)n_contigs * K, 0);
    span_sum.assign((size_t)n_contigs * K, 0.0);
    std::map<std::pair<int, int>, int> gmap;   // (kid, span) -> gid
#pragma omp parallel for schedule(dynamic)
    for (int c = 0; c < n_contigs; ++c) {
        const int *ob = obs[c];
        std::vector<int> prev;
        int prev_id = -1;
        for (int i = 0; i < Ls[c]; ++i) {
            const int *r = ob + (size_t)i * ncol;
            int id;
            if (!prev.empty() && std::equal(prev.begin(), prev.end(), r + 1)) id = prev_id;
            else {
                prev.assign(r + 1, r + ncol);
                id = kmap.find(prev)->second;
                prev_id = id;
            }
            const size_t g = (size_t)contig_base[c] + i + 1;
            rowinfo[g].kid = id;
            span_of[g] = r[0];
            present[(size_t)c * K + id] = 1;
            span_sum[(size_t)c * K + id] += (double)r[0];
        }
    }
    for (int c = 0; c < n_contigs; ++c)
        for (int i = 1; i <= Ls[c]; ++i) {
            const size_t g = (size_t)contig_base[c] + i;
            if (span_of[g] > 1) gmap.emplace(std::make_pair(rowinfo[g].kid, span_of[g]), 0);
        }
    G = (int)gmap.size();
    if (G >= (1 << 20)) throw std::runtime_error("too many distinct (span, key) pairs");
    groups.clear();
    eig_kid.clear();
    eig_of_key.assign(K, -1);
    {
        int id = 0;
        for (auto &kv : gmap) {
            kv.second = id++;
            const int kid = kv.first.first;
            if (eig_of_key[kid] < 0) { eig_of_key[kid] = (int)eig_kid.size(); eig_kid.push_back(kid); }
            groups.push_back(Group{kv.first.second, kid, eig_of_key[kid]});
        }
    }
    Ke = (int)eig_kid.size();
    for (int c = 0; c < n_contigs; ++c)
        for (int i = 1; i <= Ls[c]; ++i) {
            const size_t g = (size_t)contig_base[c] + i;
            if (span_of[g] > 1) rowinfo[g].gid = gmap[std::make_pair(rowinfo[g].kid, span_of[g])];
        }
    ss_max_span = 1;
    for (const Group &g : groups) ss_max_span = std::max(ss_max_span, g.span);
    {
        // the "hot" eigen key (most span > 1 rows; the second one: most of the rest) the chain kernels keep in registers
        std::vector<long long> cnt(std::max(1, Ke), 0);
        for (const RowInfo &ri : rowinfo)
            if (ri.gid >= 0) cnt[groups[ri.gid].eig]++;
        hot_eig = hot_eig2 = -1;
        for (int e = 0; e < Ke; ++e)
            if (hot_eig < 0 || cnt[e] > cnt[hot_eig]) hot_eig = e;
        for (int e = 0; e < Ke; ++e)
            if (e != hot_eig && (hot_eig2 < 0 || cnt[e] > cnt[hot_eig2])) hot_eig2 = e;
    }
    {
        // key slots of the scan chains: slot = frequency rank of the key (slot 0 = most rows; the emission vectors of the first
        // ChainPlan::nlds slots live in LDS)
        std::vector<long long> kc(K, 0);
        for (int c = 0; c < n_contigs; ++c)
            for (int i = 1; i <= Ls[c]; ++i) kc[rowinfo[(size_t)contig_base[c] + i].kid]++;
        std::vector<int> order(K);
        for (int k = 0; k < K; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return kc[x] > kc[y]; });
        ss_slot_of_key.assign(K, 0);
        for (int r = 0; r < K; ++r) ss_slot_of_key[order[r]] = r;
    }
}

void smcpp_im::build_device(int dev) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        throw std::runtime_error("no HIP device available: the SMC++ MI355X engine has no CPU fallback");
    if (dev >= 0) HIPCHK(hipSetDevice(dev));
    HIPCHK(hipGetDevice(&device));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&stream3, hipStreamNonBlocking));
    {
        // (the per-row gammas beside the statistics: the highest priority places their workgroups ahead of the rank updates)
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&stream_hi, hipStreamNonBlocking, greatest));
    }
    read_dual_stream();
    {
        // The events order streams of this device and bracket intervals; nothing the host reads depends on a system-scope fence at
        // an event (results reach it through stream-ordered copies and the pinned completion word of k_signal / k_fin_both).  A
        // default event makes every record a cache writeback + invalidation (hip_runtime_api.h: hipEventDisableSystemFence); an E-step
        // records about ten: headline 1 068 -> 1 082 evals/s, M = 256 2.79 -> 2.74 ms without it.  SMCPP_EVENT_FLAGS=0: default events.
        const unsigned evf = (unsigned)opt().ll(smcpp_opt::O_EVENT_FLAGS, (long long)hipEventDisableSystemFence);
        for (auto &e : ev) HIPCHK(hipEventCreateWithFlags(&e, evf));
    }
    {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        cu_count = prop.multiProcessorCount;
    }
    make_chunks();
    lay = cut_stats_layout();
    alloc_device();
    update_pi_default();
    // defaults after construction (_smcpp.pyx:318-320)
    alpha = 1.0; theta = 1e-4; rho = 1e-4;
    loglik.assign(n_contigs, 0.0);
}

// Chunks per contig of the scan chains for `nslots` wavefront slots (cost = positions, or cost units with hybrid rows): start from
// the rounded-down share of every contig and hand the remaining slots, one at a time, to the contig whose chunks are currently
// the longest - never more chunks than slots (unless there are more contigs than slots), and the longest chunk is as short as the
// slot count allows.  Host-only; exported as smcpp_host_chunk_counts for the CPU tests.
static std::vector<int> ss_chunk_counts(const std::vector<long long> &cpos, const std::vector<int> &rows, long long nslots,
                                        long long floor_cost) {
    const int n = (int)cpos.size();
    long long total = 0;
    for (long long c : cpos) total += c;
    const long long bpc = std::max<long long>(std::max<long long>(1, floor_cost), (total + nslots - 1) / std::max<long long>(1, nslots));
    std::vector<int> ncs(n, 1);
    long long used = 0;
    for (int c = 0; c < n; ++c) {
        ncs[c] = (int)std::max<long long>(1, std::min<long long>(rows[c], cpos[c] / bpc));
        used += ncs[c];
    }
    const long long want = std::max<long long>(n, std::min<long long>(nslots, (total + bpc - 1) / bpc));
    while (used < want) {
        int best = -1;
        double bl = 0.0;
        for (int c = 0; c < n; ++c) {
            if (ncs[c] >= rows[c]) continue;
            if (cpos[c] < (long long)(ncs[c] + 1) * std::max<long long>(1, floor_cost)) continue;     // no chunk below the floor
            const double len = (double)cpos[c] / ncs[c];
            if (best < 0 || len > bl) { best = c; bl = len; }
        }
        if (best < 0) break;
        ++ncs[best];
        ++used;
    }
    return ncs;
}

// The plan of the chain phase for `compute_units` compute units and the chunking the caller asked for (user_rows_per_chunk).  Reads the
// host layout and the switches, writes nothing, calls no HIP function: smcpp_host_chain_plan runs it on a machine without a device.
// `previous`: the plan this one replaces (smcpp_set_chunking) - what is fixed per manager is taken from it.
ChainPlan smcpp_im::resolve_chain_plan(int compute_units, const ChainPlan *previous) const {
    ChainPlan p;
    p.resolved = true;
    const int cus = std::max(1, compute_units);
    {
        // SMCPP_CHAIN = lock: the lock-step kernels forced (M <= 64); = dense: the cooperative kernels; ss (or unset): see below
        const char *m = opt().has(smcpp_opt::O_CHAIN) ? opt().str(smcpp_opt::O_CHAIN).c_str() : nullptr;
        if (m) p.dense = (!strcmp(m, "lock") && Mp <= 64) ? ChainPlan::LOCK_STEP : ChainPlan::COOPERATIVE;
        // lock-step chains on the matrix cores (chains_lock.hpp): 16 chunks per workgroup, so 16 x more and 16 x shorter
        // chunks - they pay off when those are still long against the ~900 rows of history every chunk re-runs
        // (rows per (CU x 16) from which they win - tools/lock_crossover.py on the whole-genome generator: M = 64 and 48 from ~400,
        // M = 32 from ~700; at M = 16 the cooperative kernels are never slower)
        const long long lock_min_rows = opt().ll(smcpp_opt::O_LOCK_MIN_ROWS, -1) >= 0 ? opt().ll(smcpp_opt::O_LOCK_MIN_ROWS, -1)
                                        : Mp >= 48 ? 450 : Mp >= 32 ? 800 : (1ll << 40);
        if (!m && Mp <= 64 && (total_rows - n_contigs) / ((long long)compute_units * LOCK_NC) >= lock_min_rows) {
            // ... and when one eigen key dominates the span > 1 rows (binned data: the monomorphic key): only its operators are
            // register-resident there, every other key present in a step costs two L2 round trips for the whole workgroup
            std::vector<long long> cnt(std::max(1, Ke), 0);
            long long ne = 0;
            for (const RowInfo &ri : rowinfo)
                if (ri.gid >= 0) { ++cnt[groups[ri.gid].eig]; ++ne; }
            const long long top = *std::max_element(cnt.begin(), cnt.end());
            if (ne == 0 || 10 * top >= 9 * ne) p.dense = ChainPlan::LOCK_STEP;
        }
        // 64 < M <= 256: the streaming cooperative kernels (k_fwd_big / k_bwd_big)
        if (Mp > 64) p.dense = ChainPlan::STREAMED_OPERANDS;
        // Chains on the semiseparable structure of T (chains_ss.hpp): one position per step, so the input qualifies when
        // its spans are short (binned data; un-binned posterior data with spans of 10^4 .. 10^5 keep the eigen kernels).
        // `dense` then names the DENSE kernels an E-step falls back to when its T has no such structure.
        const bool ss_ok = !opt().off(smcpp_opt::O_SS) && (!m || !strcmp(m, "ss")) && Mp <= 1024;
        p.scan = ss_ok && ss_max_span <= 512;
        if (ss_ok && !p.scan) {
            // longer spans: the hybrid form, when one state per lane holds the vector and the eigenvector tables of every eigen
            // key fit LDS beside the emission vectors (SMCPP_HYBRID=0: the dense kernels)
            const bool hy_off = opt().off(smcpp_opt::O_HYBRID);
            const size_t tab = (size_t)Ke * 4 * Mp * (Mp + 1) * sizeof(double);
            const bool fits = !hy_off && Mp <= 64 && Ke >= 1 && Ke <= 4;
            if (fits && tab <= 120 * 1024) p.hybrid = ChainPlan::ALL_TABLES;
            // (round 4) M > 32: four 33 KB tables per eigen key do not fit, the two a DIRECTION needs do - every workgroup
            // runs one direction (the task table keeps them apart) and stages that direction's pair
            else if (fits && tab / 2 <= 136 * 1024) p.hybrid = ChainPlan::DIRECTION_SPLIT;
            // (round 5) ... and with three or four eigen keys at M > 32 not even those: the most frequent keys keep their pair
            // in LDS, a COLD key's table rows are read from L2 on the rows that need them (chains_ss.hpp: ss_eig_matvec_cold)
            else if (fits && Mp > 32 && tab / 2 / Ke <= 136 * 1024) p.hybrid = ChainPlan::DIRECTION_SPLIT_COLD_KEYS;
            if (p.hybrid) { p.scan = true; p.hyb_th = std::max(1, opt().i(smcpp_opt::O_HYB_TH, 6)); }
            p.nk_lds = Ke;
            if (p.hybrid == ChainPlan::DIRECTION_SPLIT_COLD_KEYS) {
                // slots by frequency of the keys' hybrid rows
                std::vector<long long> cnt(Ke, 0);
                for (const RowInfo &ri : rowinfo)
                    if (ri.gid >= 0 && groups[ri.gid].span > p.hyb_th) ++cnt[groups[ri.gid].eig];
                std::vector<int> order(Ke);
                for (int e = 0; e < Ke; ++e) order[e] = e;
                std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cnt[x] > cnt[y]; });
                p.nk_lds = (int)std::max<size_t>(1, std::min<size_t>((size_t)Ke, (size_t)(136 * 1024) / (tab / 2 / Ke)));
                for (int e = 0; e < 4; ++e) p.eslot_of_key[e] = -1;
                for (int sl = 0; sl < p.nk_lds; ++sl) { p.ekey_of_slot[sl] = order[sl]; p.eslot_of_key[order[sl]] = sl; }
            }
        }
        if (p.scan) p.dense = Mp > 64 ? ChainPlan::STREAMED_OPERANDS : ChainPlan::COOPERATIVE;
        if (opt().i(smcpp_opt::O_COOP_BPC, 0) > 0) p.coop_bpc = opt().i(smcpp_opt::O_COOP_BPC, 0);
        else {
            // More workgroups per CU hide the per-row latency of the cooperative kernels (measured on 6.8 M rows:
            // throughput x1.27 / x1.36 / x1.42 for 2 / 3 / 4 per CU) but shorten the chunks, and every chunk pays
            // ~1100 rows of re-run history; the break-even points below follow from those two numbers.
            const long long per_cu = (total_rows - n_contigs) / cus;
            p.coop_bpc = per_cu < 3000 ? 1 : per_cu < 9000 ? 2 : per_cu < 17000 ? 3 : 4;
        }
    }
    // The jump key of the scan chains and whether the input jumps at all (once per manager: the row descriptors carry it, and it does
    // not depend on the chunking; chains_ss.hpp: power jumps).  SMCPP_SS_JUMP: 0 = never; 16, 8 or 4 = that power, whatever the size
    // of the input (any other value: 8); unset: power 8 on inputs of at least 200 000 positions.
    if (previous) { p.jump_kid = previous->jump_kid; p.jump_P = previous->jump_P; }
    else [&] {
    if (!p.scan || p.hybrid || NPL != 1 || opt().off(smcpp_opt::O_SS_JUMP)) return;
    int P = opt().i(smcpp_opt::O_SS_JUMP, 8);
    if (P != 16 && P != 8 && P != 4) P = 8;
    // positions in span > 1 rows per key, all positions
    std::vector<long long> kpos(K, 0);
    long long total = 0;
    for (int c = 0; c < n_contigs; ++c)
        for (int i = 1; i <= Ls[c]; ++i) {
            const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
            if (ri.gid >= 0) kpos[groups[ri.gid].kid] += groups[ri.gid].span;
            total += ri.gid < 0 ? 1 : groups[ri.gid].span;
        }
    int best = 0;
    for (int k = 1; k < K; ++k)
        if (kpos[k] > kpos[best]) best = k;
    if (K <= 0 || kpos[best] == 0) return;
    long long saved = 0;
    for (int c = 0; c < n_contigs; ++c)
        for (int i = 1; i <= Ls[c]; ++i) {
            const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
            if (ri.gid >= 0 && groups[ri.gid].kid == best) saved += std::max<long long>(0, groups[ri.gid].span - ss_jump_cost(groups[ri.gid].span, P));
        }
    if (20 * saved < total) return;
    // ... and, unless SMCPP_SS_JUMP names the power itself, on inputs of at least 200 000 positions.  Smaller inputs would gain as well
    // (6 - 8 % of chain time on the 10 000 / 20 000-position goldens) but keep the history the existing yardsticks were set on: with a few
    // chunks and keys of one row, the gamma sums of the float and the fp64 scans differ by 0.3 .. 2.3e-6 depending on which float
    // history fed them (scan steps 1.3e-6, jumps by 16 / 4 / 8: 0.3 / 0.7 / 2.3e-6; either is 1.6 .. 2.1e-6 from the reference), and
    // tests/test_gpu_parity.py holds that difference to 2e-6.  DESIGN.md section 6.
    if (!opt().has(smcpp_opt::O_SS_JUMP) && total < 200000) return;
    p.jump_kid = best; p.jump_P = P;
    }();
    // cost units (positions, or SS_HYB_COST for a hybrid row) per contig and in all
    std::vector<long long> cpos(n_contigs, 0);
    for (int c = 0; c < n_contigs; ++c) {
        for (int i = 1; i <= Ls[c]; ++i) {
            const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
            cpos[c] += ri.gid < 0 ? 1 : ss_row_cost(p, groups[ri.gid].span);
        }
        p.positions += cpos[c];
    }
    const long long total_bins = p.positions;
    if (previous) { p.wpc = previous->wpc; p.wg_waves = previous->wg_waves; p.mid = previous->mid; }   // (the by-rows cutter leaves them as they were)
    p.by_positions = p.scan && user_rows_per_chunk <= 0 && !opt().has(smcpp_opt::O_ROWS_PER_CHUNK);
    if (p.by_positions) {
        // scan chains: one wavefront per chunk and direction, a workgroup = 2 forward + 2 backward chunks = one wavefront per
        // SIMD; chunks are cut by POSITIONS (sum of spans), the unit of work of these kernels.  Every chunk pays the same
        // ~3000 positions of re-run history however short it is (the chains forget with an e-fold of ~240 positions).
        // Wavefronts per SIMD: one wavefront leaves a quarter of the issue slots empty (an instruction occupies the SIMD for 4 of
        // the ~5.3 clocks between two issues of one wavefront), a second and third fill them - but every chunk pays ~3 000 positions
        // of re-run history, so only inputs whose chunks stay long (>= 9 000 positions) take them.  Whole genome (28.7 M
        // positions): 9.3 / 8.2 / 7.9 ms of chains with 1 / 2 / 3; a 3.4 M-position shard: 1.83 / 1.95 ms with 1 / 2.
        const long long simds = (long long)compute_units * 4;
        // (round 6, last session) one state per lane, re-measured on single contigs of 150 ... 1 700 Mbp and a rank's shard of the genome
        // (gpurun_out/r06_gp12 ... gp17): between 1.95 and 12 million positions TWO wavefronts per SIMD that enter their chunks through a
        // float halo (no light passes, no fp64 part of the halo) beat one wavefront with light passes by 10 - 19 % (250 Mbp 1.66 -> 1.44 ms,
        // 700 Mbp 2.94 -> 2.46, 1 100 Mbp 4.15 -> 3.37, the 8-GPU run's shard 1.75 -> 1.57), from 12 million on three wavefronts without a
        // halo win (1 700 Mbp 6.01 -> 4.59; whole genome unchanged); below 1.35 million (the headline: 1 million) nothing changes.
        p.mid = false;
        int wpc_auto = (int)std::max<long long>(1, std::min<long long>(3, total_bins / (simds * 9000)));
        if (NPL == 1 && !p.hybrid) {
            const long long per_simd = total_bins / std::max<long long>(1, simds);
            // (... and between 1.35 and 1.95 million the halo with ONE wavefront: 135 / 150 / 175 Mbp 1.19 / 1.34 / 1.52 -> 1.12 / 1.18 / 1.27 ms;
            // at 200 Mbp the light passes hit a sweet spot - 1 + 1 of them, three launches, 1.26 ms - that the halo forms miss by 3 %:
            // the rule stays monotone, gpurun_out/r06_gp17)
            wpc_auto = per_simd >= 11700 ? 3 : per_simd >= 1900 ? 2 : 1;
            p.mid = (wpc_auto == 2 || per_simd >= 1300) && wpc_auto < 3 && !opt().has(smcpp_opt::O_SS_WPC);
        }
        p.wpc = opt().has(smcpp_opt::O_SS_WPC) ? std::max(1, std::min(4, opt().i(smcpp_opt::O_SS_WPC, 1))) : wpc_auto;
        // hybrid rows are bound by instruction and LDS LATENCY (a dependent chain of ~200 instructions per row): a second wavefront
        // per SIMD fills the gaps from ~2 000 cost units per chunk on (posterior workload: 1.79 -> 1.35 ms of chains; a third one
        // needs an extra pass: 1.80); the eight wavefronts form ONE workgroup so that the CU holds one copy of the tables
        if (p.hybrid && !opt().has(smcpp_opt::O_SS_WPC)) p.wpc = (int)std::max<long long>(1, std::min<long long>(2, total_bins / (simds * 2000)));
        if (p.hybrid) p.wpc = std::min(p.wpc, 2);
        p.wg_waves = (p.hybrid && p.wpc == 2) ? 8 : 4;
        const long long waves = simds * p.wpc;
        // Halo pass (chains_ss.hpp): with several chunks per contig every wavefront first walks into its chunk from its neighbour's
        // rows - `light` positions in float, then `dbl` in fp64, neither stored - so that ONE launch leaves rows that are already
        // exact to the certificate's tolerance (the chains forget with an e-fold of ~240 positions forward, ~340 backward: 11.5 +
        // 3.3 e-folds), instead of two store-free light passes over the WHOLE chunk, a full pass and a merge re-run.
        // Measured (profiles/r04_e_halo_probe.log): on one 100 Mbp contig at M <= 64 the halo is as long as two chunks - the same
        // history the two light passes walk - so it only trades the merge re-run against chunks of unequal length: 0.92 ms against
        // 0.87; with several states per lane (M > 64), where a light position costs relatively more, it wins (c5: 1.45 against 1.64 ms).
        // Default: M > 64 only; SMCPP_SS_HALO = 1 / 0 forces it.
        // (the mid-size regime of one state per lane, above: halo on, float part only)
        p.halo = !p.hybrid && (opt().has(smcpp_opt::O_SS_HALO) ? opt().i(smcpp_opt::O_SS_HALO, 0) != 0 : (NPL >= 2 || p.mid));
        const bool mid_halo = p.halo && p.mid && NPL == 1;
        const long long hlf = p.halo ? opt().ll(smcpp_opt::O_HALO_LF, 2800) : 0, hdf = p.halo ? opt().ll(smcpp_opt::O_HALO_DF, mid_halo ? 0 : 800) : 0,
                        hlb = p.halo ? opt().ll(smcpp_opt::O_HALO_LB, 3900) : 0, hdb = p.halo ? opt().ll(smcpp_opt::O_HALO_DB, mid_halo ? 0 : 1100) : 0;
        p.halo_lf = hlf; p.halo_df = hdf; p.halo_lb = hlb; p.halo_db = hdb;
        {
            // the forward chain gets SMCPP_SS_FWD_SHARE of the wavefronts.  Default one half: the backward chain's light position
            // costs 38 instructions against 25, but the fp64 passes of the two directions take the same time (forward: stores, the
            // reciprocal and the feedback of the stored vector per row), and measured on the headline 0.45 / 0.42 / 0.38 / 0.34 lose
            // 6 / 12 / 28 / 37 % of chain time against 0.5
            // (halo pass: the backward wavefronts carry the longer halo and the dearer position, so they get more, shorter chunks:
            // per wavefront halo_f + 53 P / c_f = halo_b + 59 P / c_b instructions with c_f + c_b = waves)
            double dflt_share = 0.5;
            if (p.halo && total_bins > 0) {
                const double Hf = 25.0 * hlf + 53.0 * hdf, Hb = 29.0 * hlb + 59.0 * hdb, P = (double)total_bins, W = (double)waves;
                double lo = 0.05, hi = 0.95;
                for (int it = 0; it < 40; ++it) {
                    const double m = 0.5 * (lo + hi);
                    const double f = Hf + 53.0 * P / (m * W), b = Hb + 59.0 * P / ((1.0 - m) * W);
                    if (f > b) lo = m; else hi = m;
                }
                dflt_share = std::min(0.5, std::max(0.25, 0.5 * (lo + hi)));
                // (one state per lane, float halo only: the stored passes of the two directions cost the same since round 5 and the task
                // table pairs them on the SIMDs one to one - 0.30 ... 0.58 measured on 175 ... 1 100 Mbp, gpurun_out/r06_gp22 / gp23: one half
                // is the optimum, 0 - 3 % ahead of the balance above, whose per-position costs are those of several states per lane)
                if (mid_halo) dflt_share = 0.5;
            }
            p.fwd_share = opt().d(smcpp_opt::O_SS_FWD_SHARE, dflt_share);
            p.waves_fwd = std::max<long long>(1, (long long)(p.fwd_share * (double)waves + 0.5));
            p.waves_bwd = std::max<long long>(1, waves - p.waves_fwd);
        }
        // Chunks per contig: NEVER more chunks than wavefront slots in total (a launch of 1046 wavefronts on 1024 SIMDs puts two
        // on some of them, and the kernel then lasts as long as those take: whole genome, 22 contigs each rounded up, +27 %).
        // Start from the rounded-down share of every contig and hand the remaining slots, one at a time, to the contig whose
        // chunks are currently the longest (minimises the longest chunk).  No chunk below 1 024 positions.
        p.chunks_fwd = ss_chunk_counts(cpos, Ls, p.waves_fwd, 1024);
        p.chunks_bwd = ss_chunk_counts(cpos, Ls, p.waves_bwd, 1024);
    } else {
        // chunks in flight: one per SIMD for the per-wavefront kernels, coop_bpc per CU for the cooperative ones
        const long long slots = (long long)compute_units *
                                (p.dense == ChainPlan::LOCK_STEP ? LOCK_NC : p.dense == ChainPlan::STREAMED_OPERANDS ? 1 : p.coop_bpc);
        const long long rows = total_rows - n_contigs;
        int lc = user_rows_per_chunk;
        if (lc <= 0) lc = opt().i(smcpp_opt::O_ROWS_PER_CHUNK, lc);
        // every chunk pays ~1000 rows of re-run history however short it is, so small inputs get few, long chunks rather
        // than one sliver per CU (a 1 500-row contig: 3 chunks and 4 passes instead of 24 chunks and 15 passes)
        if (lc <= 0) lc = (int)std::max<long long>(512, (rows + slots - 1) / slots);
        p.rows_per_chunk = lc;
        p.chunks_fwd.resize(n_contigs);
        for (int c = 0; c < n_contigs; ++c) p.chunks_fwd[c] = std::max(1, ceil_div(Ls[c], lc));
        p.chunks_bwd = p.chunks_fwd;             // (the backward list is a copy of the forward one: no halo on this path)
    }
    for (int c = 0; c < n_contigs; ++c) p.max_chunks_per_contig = std::max(p.max_chunks_per_contig, std::max(p.chunks_fwd[c], p.chunks_bwd[c]));
    p.max_pass = p.max_chunks_per_contig + 3;    // (+1: the full pass that follows an eigen-free pre-pass)
    if (p.scan) p.max_pass += 4 + 2;             // (+4: light passes, +2: a warm start numbers its passes from 1 or 2)
    // the emission vectors of the first nlds key slots live in LDS; the instantiation of k_chain_ss follows from it: every key slot
    // in LDS (the usual case) is the one without the global path of the emission vectors, and at M <= 32 with one state per lane
    // and no hybrid rows its scans skip the level that would only move zeros (SMCPP_SS_H32=0: the full-width form there too)
    // (fixed at construction; wpc workgroups share a CU's 160 KB, the hybrid form runs one workgroup per CU beside its tables.
    // Until round 5 the table was capped at 64 KB: the 192 six-int keys of config C4 - 96 KB at M = 48 - left 64 slots to the L2 path
    // and with them the kernel to its instantiation with vector-memory waits on every row: chains 0.86 -> see DESIGN.md section 6)
    const long long slot_bytes = 64 * NPL * 8;
    if (previous) p.nlds = previous->nlds;
    else if (p.hybrid) p.nlds = (int)std::max<long long>(1, std::min<long long>(K, (long long)((p.dirsplit() ? 158 : 150) * 1024 - ss_tab_bytes(p, Mp)) / slot_bytes));
    else p.nlds = (int)std::min<long long>(K, ((150 / std::max(1, p.wpc)) * 1024) / slot_bytes);
    p.all_keys_in_lds = K <= p.nlds;
    p.two_row_scans = NPL == 1 && !p.hybrid && p.all_keys_in_lds && Mp <= 32 && !opt().off(smcpp_opt::O_SS_H32);
    {
        // Eigen-free pre-pass of the dense families: spans below 32 (binned data: four squarings give every power); chunks short
        // enough that pass 1 re-runs them whole anyway (the rows of the pre-pass are all overwritten: it runs in float and its
        // normalisers carry no eigenvalue scale)
        int mx = 0, longest = 0;
        for (int g = 0; g < G; ++g) mx = std::max(mx, groups[g].span);
        if (!p.by_positions)
            for (int c = 0; c < n_contigs; ++c)
                for (int j = 0, nc = p.chunks_fwd[c]; j < nc; ++j)
                    longest = std::max(longest, (int)((long long)Ls[c] * (j + 1) / nc) - (int)((long long)Ls[c] * j / nc));
        const char *pe = opt().has(smcpp_opt::O_POWER_PREPASS) ? opt().str(smcpp_opt::O_POWER_PREPASS).c_str() : nullptr;
        const bool coop_pre = p.dense == ChainPlan::COOPERATIVE && Mp <= 64;
        const bool big_pre = p.dense == ChainPlan::STREAMED_OPERANDS && Mp > 64 && Mp <= 256;
        // spans up to twelve bits (4095 positions); the cooperative chains read the powers beyond A^16 from L2 on the few rows
        // that need them, the streamed-operand ones stream every power anyway
        p.power_ok = (coop_pre || big_pre) && mx <= 4095 && Ke >= 1 && G >= 1 && longest <= 2000 && !(pe && atoi(pe) == 0) && !p.scan;
        p.max_span_pw = mx;
        while ((1 << p.pw_nbits) <= mx) ++p.pw_nbits;
        p.pw_npow = p.pw_nbits - 1;
    }
    return p;
}

// The two chunk lists of a plan: by positions with halos (the automatic chunking of the scan chains), or by rows.  Decides nothing.
void smcpp_im::cut_chunks(const ChainPlan &p) {
    max_chunks_per_contig = p.max_chunks_per_contig;
    if (!p.by_positions) {
        chunks.clear();
        for (int c = 0; c < n_contigs; ++c) {
            const int L = Ls[c], nc = p.chunks_fwd[c];
            for (int j = 0; j < nc; ++j) {
                Chunk ch;
                ch.base = contig_base[c];
                ch.r0 = (int)((long long)L * j / nc);
                ch.r1 = (int)((long long)L * (j + 1) / nc);
                ch.contig = c;
                ch.first = (j == 0);
                ch.last = (j == nc - 1);
                ch.pad = 0;
                ch.h0 = ch.h1 = ch.r0;               // (forward list; the backward copy below is given r1: no halo on this path)
                chunks.push_back(ch);
            }
        }
        chunks_b = chunks;
        for (Chunk &cb : chunks_b) cb.h0 = cb.h1 = cb.r1;
        return;
    }
    std::vector<long long> cum;
    auto cut = [&](const std::vector<int> &ncs, std::vector<Chunk> &out, bool bwd, long long halo_l, long long halo_d) {
        out.clear();
        for (int c = 0; c < n_contigs; ++c) {
            const int L = Ls[c];
            cum.assign((size_t)L + 1, 0);
            for (int i = 1; i <= L; ++i) {
                const RowInfo &ri = rowinfo[(size_t)contig_base[c] + i];
                cum[i] = cum[i - 1] + (ri.gid < 0 ? 1 : ss_row_cost(p, groups[ri.gid].span));
            }
            const int nc = ncs[c];
            int prev = 0;
            for (int j = 0; j < nc; ++j) {
                int r1;
                if (j == nc - 1) r1 = L;
                else {
                    const long long target = cum[L] * (j + 1) / nc;
                    r1 = (int)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
                    r1 = std::max(prev + 1, std::min(r1, L - (nc - 1 - j)));
                }
                Chunk ch;
                ch.base = contig_base[c];
                ch.r0 = prev; ch.r1 = r1; ch.contig = c;
                ch.first = (j == 0); ch.last = (j == nc - 1); ch.pad = 0;
                // halo rows (positions counted on this contig's cumulative costs): forward chunks look back, backward ones ahead
                if (bwd) {
                    const long long e1 = cum[r1] + halo_d, e0 = e1 + halo_l;
                    ch.h1 = (int)std::min<long long>(L, std::lower_bound(cum.begin(), cum.end(), e1) - cum.begin());
                    ch.h0 = (int)std::min<long long>(L, std::lower_bound(cum.begin(), cum.end(), e0) - cum.begin());
                    if (halo_l + halo_d == 0 || ch.last) ch.h0 = ch.h1 = r1;
                } else {
                    const long long e1 = cum[prev] - halo_d, e0 = e1 - halo_l;
                    ch.h1 = e1 <= 0 ? 0 : (int)(std::upper_bound(cum.begin(), cum.end(), e1) - cum.begin()) - 1;
                    ch.h0 = e0 <= 0 ? 0 : (int)(std::upper_bound(cum.begin(), cum.end(), e0) - cum.begin()) - 1;
                    ch.h1 = std::min(ch.h1, prev); ch.h0 = std::min(ch.h0, ch.h1);
                    if (halo_l + halo_d == 0 || ch.first) ch.h0 = ch.h1 = prev;
                }
                out.push_back(ch);
                prev = r1;
            }
        }
    };
    cut(p.chunks_fwd, chunks, false, p.halo_lf, p.halo_df);
    cut(p.chunks_bwd, chunks_b, true, p.halo_lb, p.halo_db);
}

void smcpp_im::upload_chunk_state() {
    ss_warm_valid = false;
    const size_t nch = std::max(chunks.size(), chunks_b.size());
    d_chunks.upload(chunks, stream);
    d_chunks_b.upload(chunks_b, stream);
    {
        // wavefront -> (direction, chunk) of the one-chain-per-wavefront launches: the two directions interleaved in proportion, so
        // that every workgroup (4 wavefronts = the 4 SIMDs of a CU) holds its share of both
        const size_t nf = chunks.size(), nb = chunks_b.size();
        ss_tasks.clear();
        size_t i = 0, j = 0;
        if (plan.dirsplit()) {
            // single-direction workgroups, the two kinds interleaved in proportion
            const size_t W = (size_t)plan.wg_waves;
            while (i < nf || j < nb) {
                const bool take_f = j >= nb || (i < nf && (double)i * (double)nb <= (double)j * (double)nf);
                for (size_t q = 0; q < W; ++q) {
                    if (take_f) ss_tasks.push_back(i < nf ? (int)i++ : -1);
                    else ss_tasks.push_back(j < nb ? ((1 << 30) | (int)j++) : -1);
                }
            }
        } else
        while (i < nf || j < nb) {
            // next task: the direction that is behind its proportional share
            const bool take_f = j >= nb || (i < nf && (double)i * (double)nb <= (double)j * (double)nf);
            if (take_f) ss_tasks.push_back((int)i++);
            else ss_tasks.push_back((1 << 30) | (int)j++);
        }
        while (ss_tasks.size() % plan.wg_waves) ss_tasks.push_back(-1);
        d_tasks.upload(ss_tasks, stream);
    }
    d_ends_f.alloc(2 * nch * Mp); d_used_f.alloc(nch * Mp);
    d_ends_b.alloc(2 * nch * Mp); d_used_b.alloc(nch * Mp);
    d_changed_f.alloc(plan.max_pass + 1); d_changed_b.alloc(plan.max_pass + 1);
    HIPCHK(hipStreamSynchronize(stream));
}

// pi of defaultEta (a = s = {1}: R(t) = t), inference_manager.cpp:12-19,43,56-69: what a fresh HMM's statistics hold; follows
// the hidden states (smcpp_set_hidden_states before the first E-step)
void smcpp_im::update_pi_default() {
    pi_default.assign(M, 0.0);
    double sm = 0.0;
    for (int m = 0; m < M; ++m) {
        double v = std::exp(-hs[m]) - ((m + 1 < M) ? std::exp(-hs[m + 1]) : 0.0);
        if (v < 1e-20) v = 1e-20;
        pi_default[m] = v;
        sm += v;
    }
    for (double &v : pi_default) v /= sm;
}

static bool stats_team_on() { return !opt().off(smcpp_opt::O_STATS_TEAM); }

// The layout of the statistics: reads the row layout (rowinfo, groups, contig_base, Ls, the shape) and the switches SMCPP_SLAB_ROWS and
// SMCPP_STATS_TEAM, writes nothing else, calls no HIP function: smcpp_host_stats_plan runs it on a machine without a device.
StatsLayout smcpp_im::cut_stats_layout() const {
    StatsLayout L;
    auto &perm1 = L.perm1.h, &perme = L.perme.h, &gk_slab_off = L.gk_slab_off.h, &s1_slab_off = L.s1_slab_off.h, &eb_slab_off = L.eb_slab_off.h,
         &eb_gid = L.eb_gid.h, &ce_bucket_off = L.ce_bucket_off.h, &ce_row_off = L.ce_row_off, &erow_slab = L.erow_slab.h, &fk_c_off = L.fk_c_off.h,
         &fk_gk_off = L.fk_gk_off.h, &ek_slab_off = L.ek_slab_off.h, &epos_gid = L.epos_gid.h;
    auto &perm1k = L.perm1k.h; auto &erow_desc = L.erow_desc.h;
    auto &slabs_sc = L.slabs_sc.h, &slabs_rk = L.slabs_rk.h, &slabs_eg = L.slabs_eg.h, &slabs_fk = L.slabs_fk.h, &slabs_ek = L.slabs_ek.h;
    // counting sorts of rows per contig
    gk_slab_off.assign((size_t)n_contigs * K + 1, 0);
    s1_slab_off.assign(n_contigs + 1, 0);
    ce_bucket_off.assign((size_t)n_contigs * Ke + 1, 0);
    ce_row_off.assign((size_t)n_contigs * Ke + 1, 0);
    int last_eig_key = -1;
    long long n1 = 0, ne = 0;
    // (rows with ell = 0 have kid = 0, gid = -1 and are skipped below)
    for (int c = 0; c < n_contigs; ++c)
        for (int i = 1; i <= Ls[c]; ++i) (rowinfo[(size_t)contig_base[c] + i].gid < 0 ? n1 : ne)++;
    L.n_1_rows = n1; L.n_e_rows = ne;
    const long long part_bytes = (long long)Mp * Mp * 8;
    // slabs = independent single-wavefront work items; several thousand keep the 2048 resident wavefronts of the
    // chip balanced on large inputs (each slab owns an Mp x Mp partial: at most 256 MB of them)
    // (round 5: teams of four slabs share one partial - k_rank_acc<., true> -, so four times as many slabs fit the same 256 MB)
    L.teams = stats_team_on();
    const long long target = std::max<long long>(256, std::min<long long>(8192, ((L.teams ? 1024ll : 256ll) << 20) / part_bytes));
    // (at least SMCPP_SLAB_ROWS rows per slab, default 128: every slab costs an Mp x Mp partial written and read back - 128 MB of
    // traffic per headline E-step with 64-row slabs -, but a slab is walked by ONE wavefront, and below ~1000 slabs the rank
    // kernels leave SIMDs idle: 64 .. 192 rows measured: 633 / 641 / 666 / 665 headline evals per second)
    const int slab_rows = opt().has(smcpp_opt::O_SLAB_ROWS) ? std::max(16, opt().i(smcpp_opt::O_SLAB_ROWS, 128)) : 128;
    int S_RK = (int)std::max<long long>(slab_rows, (n1 + target - 1) / target);
    S_RK = (S_RK + 3) / 4 * 4;
    int S_EG = (int)std::max<long long>(slab_rows, (ne + target - 1) / target);
    S_EG = (S_EG + 15) / 16 * 16;
    const int S_SC = 256;
    L.slab_rows_1 = S_RK; L.slab_rows_e = S_EG;
    for (int c = 0; c < n_contigs; ++c) {
        const long long base = contig_base[c];
        // ---- span-1 rows sorted by key ----
        std::vector<std::vector<int>> by_key(K);
        std::vector<std::vector<int>> by_grp(G);
        for (int i = 1; i <= Ls[c]; ++i) {
            const RowInfo &ri = rowinfo[(size_t)base + i];
            if (ri.gid < 0) by_key[ri.kid].push_back(i);
            else by_grp[ri.gid].push_back(i);
        }
        const int seg_start = (int)perm1.size();
        for (int k = 0; k < K; ++k) {
            gk_slab_off[(size_t)c * K + k] = (int)slabs_sc.size();
            const int s0 = (int)perm1.size();
            perm1.insert(perm1.end(), by_key[k].begin(), by_key[k].end());
            for (int ell : by_key[k]) perm1k.push_back(make_int2(ell, k));
            const int s1 = (int)perm1.size();
            for (int s = s0; s < s1; s += S_SC)
                slabs_sc.push_back(Slab{s, std::min(s + S_SC, s1), c * K + k, k, base});
        }
        const int seg_end = (int)perm1.size();
        // the rank update does not need key-homogeneous slabs (the key only selects an L2-resident emission vector):
        // its copy of the permutation runs in natural row order, so every slab streams through alpha / beta
        std::sort(perm1k.begin() + seg_start, perm1k.begin() + seg_end,
                  [](const int2 &x, const int2 &y) { return x.x < y.x; });
        s1_slab_off[c] = (int)slabs_rk.size();
        for (int s = seg_start; s < seg_end; s += S_RK)
            slabs_rk.push_back(Slab{s, std::min(s + S_RK, seg_end), c, -1, base});
        // ---- eigen rows sorted by (eigen key, group) ----
        for (int e = 0; e < Ke; ++e) {
            ce_bucket_off[(size_t)c * Ke + e] = (int)eb_gid.size();
            ce_row_off[(size_t)c * Ke + e] = (int)perme.size();
            for (int g = 0; g < G; ++g) {
                if (groups[g].eig != e || by_grp[g].empty()) continue;
                // the fused eigen kernel shares one LDS copy of (Pinv, P) among the 4 slabs of a workgroup: pad with
                // empty slabs (they add zero partials to the previous bucket) so that no workgroup mixes eigen keys
                if (!slabs_eg.empty() && last_eig_key != e) {
                    while (slabs_eg.size() % 4 != 0) {
                        Slab pad = slabs_eg.back();
                        pad.start = pad.end;
                        slabs_eg.push_back(pad);
                    }
                }
                last_eig_key = e;
                eb_slab_off.push_back((int)slabs_eg.size());
                eb_gid.push_back(g);
                const int s0 = (int)perme.size();
                perme.insert(perme.end(), by_grp[g].begin(), by_grp[g].end());
                const int s1 = (int)perme.size();
                for (int s = s0; s < s1; s += S_EG) {
                    const int se = std::min(s + S_EG, s1);
                    for (int r = s; r < se; ++r) erow_slab.push_back((int)slabs_eg.size());
                    slabs_eg.push_back(Slab{s, se, (int)eb_gid.size() - 1, g, base});
                }
            }
        }
    }
    gk_slab_off[(size_t)n_contigs * K] = (int)slabs_sc.size();
    s1_slab_off[n_contigs] = (int)slabs_rk.size();
    ce_bucket_off[(size_t)n_contigs * Ke] = (int)eb_gid.size();
    ce_row_off[(size_t)n_contigs * Ke] = (int)perme.size();
    eb_slab_off.push_back((int)slabs_eg.size());
    // single-key span-1 slabs in key-sorted order (k_rank_acc<3>)
    fk_c_off.assign(n_contigs + 1, 0);
    fk_gk_off.assign((size_t)n_contigs * K + 1, 0);
    for (int c = 0; c < n_contigs; ++c) {
        fk_c_off[c] = (int)slabs_fk.size();
        for (int k = 0; k < K; ++k) {
            fk_gk_off[(size_t)c * K + k] = (int)slabs_fk.size();
            const int g0 = gk_slab_off[(size_t)c * K + k], g1 = gk_slab_off[(size_t)c * K + k + 1];
            if (g1 <= g0) continue;
            const int q0 = slabs_sc[g0].start, q1 = slabs_sc[g1 - 1].end;       // the (contig, key) segment of perm1
            for (int q = q0; q < q1; q += S_RK) slabs_fk.push_back(Slab{q, std::min(q + S_RK, q1), c, k, contig_base[c]});
        }
    }
    fk_c_off[n_contigs] = (int)slabs_fk.size();
    fk_gk_off[(size_t)n_contigs * K] = (int)slabs_fk.size();
    {
        auto cut = [](const std::vector<int> &range_off, std::vector<int2> &teams, std::vector<int> &team_off) {
            teams.clear();
            team_off.assign(range_off.size(), 0);
            for (size_t r = 0; r + 1 < range_off.size(); ++r) {
                team_off[r] = (int)teams.size();
                for (int q = range_off[r]; q < range_off[r + 1]; q += 4) teams.push_back(make_int2(q, std::min(4, range_off[r + 1] - q)));
            }
            if (!range_off.empty()) team_off.back() = (int)teams.size();
        };
        cut(fk_c_off, L.teams_fk.h, L.fk_c_team_off.h);
        cut(eb_slab_off, L.teams_eg.h, L.eb_team_off.h);
        cut(s1_slab_off, L.teams_rk.h, L.s1_team_off.h);
    }
    // generation-2 eigen slabs: the sorted eigen rows of every (contig, eigen key) cut into S_EG-row pieces regardless of the span
    // groups; padded like slabs_eg so that a workgroup of four never mixes keys
    ek_slab_off.assign((size_t)n_contigs * Ke + 1, 0);
    epos_gid.reserve(perme.size());
    for (size_t q = 0; q < erow_slab.size(); ++q) epos_gid.push_back(slabs_eg[erow_slab[q]].aux);
    erow_desc.reserve(perme.size());
    for (size_t q = 0; q < erow_slab.size(); ++q) {
        const Slab &sl = slabs_eg[erow_slab[q]];
        const long long row = sl.base + perme[q];
        erow_desc.push_back(make_int4((int)(row & 0xffffffffll), (int)(row >> 32), sl.aux, groups[sl.aux].span));
        L.pieces += (groups[sl.aux].span + 63) / 64;             // (the eigen-power pieces of save_gamma: at most 64 positions each)
    }
    for (int c = 0; c < n_contigs; ++c)
        for (int e = 0; e < Ke; ++e) {
            const size_t ce = (size_t)c * Ke + e;
            const int q0 = ce_row_off[ce], q1 = ce_row_off[ce + 1];
            if (q1 > q0) while (slabs_ek.size() % 4 != 0) { Slab pad = slabs_ek.back(); pad.start = pad.end; slabs_ek.push_back(pad); }
            ek_slab_off[ce] = (int)slabs_ek.size();
            for (int q = q0; q < q1; q += S_EG) slabs_ek.push_back(Slab{q, std::min(q + S_EG, q1), (int)ce, e, contig_base[c]});
        }
    // (a padding slab sits in front of the first slab of the next key: it belongs to the PREVIOUS (contig, key)'s range only if
    // that range is recorded after it, so ranges are closed here, over the padded list)
    ek_slab_off[(size_t)n_contigs * Ke] = (int)slabs_ek.size();
    {
        // blocks per contig of the log-likelihood reduction: ~2 000 rows each (64 blocks took 0.13 ms on a contig of a million rows)
        int maxL = 0;
        for (int c = 0; c < n_contigs; ++c) maxL = std::max(maxL, Ls[c]);
        L.llblk = std::max(64, std::min(1024, (maxL + 2047) / 2048));
    }
    // shares of the cross-slab reduction of the span-1 rank partials: few contigs, small M -> more, shorter shares (one contig at M = 64:
    // 8 shares of 126 slabs took 38 us of dependent loads)
    L.ZS = (int)std::max<long long>(8, std::min<long long>(16, 2048 / std::max<long long>(1, (long long)n_contigs * ceil_div((long long)Mp * Mp, 256))));
    // (the monomorphic key alone holds half the span-1 slabs of a contig: one block walking them took 42 us on the headline)
    L.ZG = (int)std::max<long long>(1, std::min<long long>(16, 1024 / std::max<long long>(1, (long long)n_contigs * K)));
    return L;
}

// the operand buffers of the eigen-free pre-pass, where the plan takes it (ChainPlan::power_ok)
void smcpp_im::setup_power() {
    if (!plan.power_ok) return;
    if (plan.dense == ChainPlan::STREAMED_OPERANDS) {
        const size_t MM = (size_t)Mp * Mp;
        d_W.alloc((size_t)Ke * plan.pw_nbits * MM);
        d_qBf.alloc((size_t)Ke * plan.pw_nbits * MM);
        d_qBb.alloc((size_t)Ke * plan.pw_nbits * MM);
        d_pre_qTf.alloc(MM);
        d_pre_qTdT.alloc(MM);
        return;
    }
    d_Bf.alloc((size_t)Ke * plan.pw_npow * Mp * Mp);
    d_Bb.alloc((size_t)Ke * plan.pw_npow * Mp * Mp);
}

void smcpp_im::alloc_device() {
    hipStream_t s = stream;
    d_rowinfo.upload(rowinfo, s);
    {
        // packed descriptors of the chain kernels
        // ROWDESC_PAD span-1 descriptors of key 0 on both sides: the chain kernels prefetch descriptors up to 192 rows
        // past either end of a chunk without bounds tests (chains2.hpp)
        std::vector<int2> rd((size_t)total_rows + 2 * ROWDESC_PAD, make_int2(0, -1));
        for (size_t r = 0; r < (size_t)total_rows; ++r) {
            const RowInfo &ri = rowinfo[r];
            rd[ROWDESC_PAD + r].x = ri.kid;
            rd[ROWDESC_PAD + r].y = ri.gid < 0 ? -1 : (ri.gid | (groups[ri.gid].eig << 20));
        }
        d_rowdesc.upload(rd, s);
        HIPCHK(hipStreamSynchronize(s));
    }
    {
        // scan chains: descriptors {key slot, span} (slot: ss_slot_of_key, build_layout); same padding as above with span-1 rows of slot 0
        // (the scan chains request one descriptor per row, two rows ahead: they read two rows past either end of a contig and
        // consume none of them)
        if (plan.scan) {
            std::vector<int2> rd((size_t)total_rows + 2 * ROWDESC_PAD, make_int2(0, 1));
            for (size_t r = 0; r < (size_t)total_rows; ++r) {
                const RowInfo &ri = rowinfo[r];
                // (upper 16 bits of x: the eigen key of a span > 1 row, read by the hybrid rows only)
                rd[ROWDESC_PAD + r] = make_int2(ss_slot_of_key[ri.kid] | ((ri.gid < 0 ? 0 : groups[ri.gid].eig) << 16), ri.gid < 0 ? 1 : groups[ri.gid].span);
            }
            // (round 6) a row that CONTINUES the caller's row of the row before it (long rows cut into pieces, build()): the vector
            // stored where it begins is not one the reference stores - no 1e-10 floor there (SS_ROW_CONT; chains_ss.hpp)
            if (split_spans)
                for (int c = 0; c < n_contigs; ++c)
                    for (int ell = 2; ell <= Ls[c]; ++ell)
                        if (piece_row[c][ell] == piece_row[c][ell - 1]) rd[ROWDESC_PAD + (size_t)contig_base[c] + ell].x |= SS_ROW_CONT;
            // rows of the jump key with room for a jump behind their first position (SS_ROW_JUMP: one scalar bit test per row in the kernel)
            if (plan.jump_P)
                for (size_t r = 0; r < (size_t)total_rows; ++r) {
                    const RowInfo &ri = rowinfo[r];
                    if (ri.gid >= 0 && groups[ri.gid].kid == plan.jump_kid && groups[ri.gid].span - 1 >= plan.jump_P) rd[ROWDESC_PAD + r].x |= SS_ROW_JUMP;
                }
            d_rowdesc_ss.upload(rd, s);
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    upload_chunk_state();
    lay.upload(s);
    d_contig_base.upload(contig_base, s);
    d_contig_L.upload(Ls, s);
    std::vector<int> gs(G), ge(G);
    for (int g = 0; g < G; ++g) { gs[g] = groups[g].span; ge[g] = groups[g].eig; }
    d_g_span.upload(gs, s);
    d_g_eig.upload(ge, s);
    d_e_kid.upload(eig_kid, s);
    setup_power();
    d_alpha.alloc((size_t)total_rows * Mp);
    d_beta.alloc((size_t)total_rows * Mp);
    d_cnorm.alloc((size_t)total_rows);
    d_logc.alloc((size_t)total_rows);
    d_w1.alloc((size_t)total_rows);
    d_llpart.alloc((size_t)n_contigs * lay.llblk);
    d_loglik.alloc(n_contigs);
    d_gpart.alloc(std::max<size_t>(1, lay.slabs_sc.h.size()) * Mp);
    // omega*U and W of the eigen rows only go through memory when the fused kernel cannot be used (M > 64)
    d_Xs.alloc(NT <= 4 ? 1 : std::max<size_t>(1, (size_t)lay.n_e_rows) * Mp);
    d_Ys.alloc(NT <= 4 ? 1 : std::max<size_t>(1, (size_t)lay.n_e_rows) * Mp);
    // (what follows from an E-step's plan is sized there, size_stats_buffers: un-binned data have 10^5 span groups and never take the per-group paths at M <= 64)
    d_red_1.alloc((size_t)n_contigs * lay.ZS * Mp * Mp);
    d_red_g.alloc((size_t)n_contigs * K * Mp * lay.ZG);
    d_Z.alloc(std::max<size_t>(1, (size_t)n_contigs * Ke) * Mp * Mp);
    d_Y.alloc(std::max<size_t>(1, (size_t)n_contigs * Ke) * Mp * Mp);
    d_xisum.alloc((size_t)n_contigs * Mp * Mp);
    d_gsum.alloc((size_t)n_contigs * K * Mp);
    d_gamma0.alloc((size_t)n_contigs * Mp);
    d_E.alloc((size_t)K * Mp);
    d_dpow.alloc(std::max<size_t>(1, (size_t)G) * Mp);
    d_g_scale.alloc(std::max(1, G));
    d_g_logscale.alloc(std::max(1, G));
    d_pi_f.alloc(Mp);
    d_Tf.alloc((size_t)Mp * Mp);
    d_TdT.alloc((size_t)Mp * Mp);
    d_Td.alloc((size_t)Mp * Mp);
    const size_t em = std::max<size_t>(1, (size_t)Ke) * Mp * Mp;
    d_PinvT.alloc(em); d_PT.alloc(em); d_Prm.alloc(em); d_Pinvrm.alloc(em);
    d_dsc.alloc(std::max<size_t>(1, (size_t)Ke) * Mp);
    d_dun.alloc(std::max<size_t>(1, (size_t)Ke) * Mp);
    // zero the row state once so padded lanes / unused rows hold finite values
    d_alpha.zero(s); d_beta.zero(s); d_cnorm.zero(s); d_logc.zero(s); d_w1.zero(s);
    HIPCHK(hipStreamSynchronize(s));
}

