/* smcpp_engine.h — C ABI of the MI355X-native SMC++ E-step engine (libsmcpp_engine.so).
 *
 * This is the drop-in boundary for the reference's Cython binding (smcpp/_smcpp.pyx + _smcpp.pxd): every entry
 * point below replaces one member of the C++ classes that `_smcpp.pxd:41-70` declares to Cython.  Opaque handle,
 * plain pointers and sizes, int status (0 = ok, nonzero = error with smcpp_last_error() holding the what()-string
 * the reference would have thrown as std::runtime_error -> Python RuntimeError, `_smcpp.pxd:43-52`).
 *
 * Matrix arguments are C-contiguous row-major doubles unless stated otherwise (the layout `store_matrix`,
 * src/common.cpp:8-11, hands to numpy).  Observation arrays are int32 [L x (1+3P)] rows (span, (a,b,nb) x P),
 * exactly what `InferenceManager::map_obs` (src/inference_manager.cpp:180-188) maps; they are copied to the
 * device at construction and need not outlive the call.
 *
 * Thread safety: an instance is used from one host thread at a time (as in the reference);
 * different instances are independent.  Every call may be made with the Python GIL released.
 */
#ifndef SMCPP_ENGINE_H
#define SMCPP_ENGINE_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smcpp_im smcpp_im;

/* Thread-local message of the last failing call on this thread. */
const char *smcpp_last_error(void);

/* ---- construction / destruction -------------------------------------------------------------------------- */

/* OnePopInferenceManager(n, obs_lengths, observations, hidden_states, polarization_error)
 * include/inference_manager.h:130-139, src/inference_manager.cpp:506-516; bound at _smcpp.pyx:312-320.
 * hs has n_hs = M+1 ascending entries (last may be +inf).  device < 0 selects the current HIP device. */
int smcpp_create_onepop(int n, int n_contigs, const int *Ls, const int *const *obs,
                        int n_hs, const double *hs, double polarization_error, int device, smcpp_im **out);

/* TwoPopInferenceManager(n1, n2, a1, a2, ...)  include/inference_manager.h:141-157,
 * src/inference_manager.cpp:518-540; bound at _smcpp.pyx:338-351.  Requires a1 + a2 == 2 and (a1,a2) != (0,2). */
int smcpp_create_twopop(int n1, int n2, int a1, int a2, int n_contigs, const int *Ls, const int *const *obs,
                        int n_hs, const double *hs, double polarization_error, int device, smcpp_im **out);

/* delete im  (_smcpp.pyx:154-155) */
void smcpp_destroy(smcpp_im *im);

/* ---- parameters ----------------------------------------------------------------------------------------- */

/* InferenceManager::setTheta / setRho / setAlpha  (src/inference_manager.cpp:71-87): mark dirty only. */
int smcpp_set_theta(smcpp_im *im, double theta);
int smcpp_set_rho(smcpp_im *im, double rho);
int smcpp_set_alpha(smcpp_im *im, double alpha);

/* InferenceManager::setParams(ParameterVector)  (src/inference_manager.cpp:256-260, _smcpp.pyx:66-83,327-332).
 * a[K] piece sizes, s[K] piece lengths; da[K x nder] forward-mode derivative seeds of a (may be NULL, nder = 0). */
int smcpp_set_params(smcpp_im *im, int K, const double *a, const double *da, int nder, const double *s);

/* Raw-parameter entry (extension, SURVEY.md §7 design note): hand the engine the products of the cold host
 * preparation directly — pi[M], T[M x M], and one emission vector per key (keys [K x 3P] int32, E [K x M]).
 * Every key that occurs in the observations must be present.  Replaces, for one E-step, what
 * do_dirty_work() (src/inference_manager.cpp:213-229) would have recomputed. */
int smcpp_set_raw(smcpp_im *im, const double *pi, const double *T, int K, const int *keys, const double *E);

/* ---- the hot path --------------------------------------------------------------------------------------- */

/* InferenceManager::Estep(bool)  (src/inference_manager.cpp:108-114 -> HMM::Estep, src/hmm.cpp:45-153). */
int smcpp_estep(smcpp_im *im, int forward_backward_only);

/* InferenceManager::loglik()  (src/inference_manager.cpp:174-177): one value per contig. */
int smcpp_loglik(smcpp_im *im, double *out);

/* InferenceManager::Q()  (src/inference_manager.cpp:116-126 -> HMM::Q, src/hmm.cpp:155-193): the four terms
 * summed over contigs; jac [4 x nder] may be NULL. */
int smcpp_q(smcpp_im *im, double val[4], double *jac);

/* Number of derivative directions the current parameters carry (nder of the last smcpp_set_params; 0 after set_raw). */
int smcpp_num_derivatives(smcpp_im *im);

/* ---- state / getters (all copy out) -------------------------------------------------------------------------- */

int smcpp_set_save_gamma(smcpp_im *im, int on);          /* InferenceManager::saveGamma, _smcpp.pyx:201-205 */
int smcpp_get_save_gamma(smcpp_im *im);
int smcpp_num_states(smcpp_im *im);                      /* M = n_hs - 1 */
int smcpp_num_contigs(smcpp_im *im);
int smcpp_num_keys(smcpp_im *im);                        /* distinct block_keys over all contigs */
int smcpp_key_len(smcpp_im *im);                         /* 3P */
int smcpp_get_hidden_states(smcpp_im *im, double *hs);   /* _smcpp.pyx:207-213 */
int smcpp_set_hidden_states(smcpp_im *im, int n_hs, const double *hs);
int smcpp_get_keys(smcpp_im *im, int *keys);             /* [K x 3P], lexicographic (block_key.h:47-56) */

int smcpp_get_xisum(smcpp_im *im, int contig, double *out);        /* getXisums(): [M x M]   */
/* getGammas(): [M x (L+1)] row-major if save_gamma was set for the last E-step, else [M x 1] */
int smcpp_get_gamma(smcpp_im *im, int contig, double *out);
/* Number of columns smcpp_get_gamma writes for this contig: L+1 if the LAST E-step ran with save_gamma, else 1
 * (the flag may have been toggled since); -1 for a bad contig index.  Size the buffer from this. */
int smcpp_gamma_cols(smcpp_im *im, int contig);
/* getGammaSums(): vals [K x M]; present[K] = 1 where the reference's std::map would hold the key */
int smcpp_get_gamma_sums(smcpp_im *im, int contig, double *vals, unsigned char *present);
int smcpp_get_pi(smcpp_im *im, double *out);                       /* getPi(): [M]           */
int smcpp_get_transition(smcpp_im *im, double *out);               /* getTransition(): [M x M] */
int smcpp_get_emission_probs(smcpp_im *im, double *out);           /* getEmissionProbs(): [K x M] */
/* Jacobians of the three getters above with respect to the derivative seeds of the last smcpp_set_params
 * (`store_matrix(const Matrix<adouble>&, double*, double*)`, src/common.cpp; _smcpp.pyx:215-275): row-major
 * [M x nder], [M*M x nder], [K*M x nder].  Nothing is written when nder == 0; an error after smcpp_set_raw. */
int smcpp_get_pi_jac(smcpp_im *im, double *out);
int smcpp_get_transition_jac(smcpp_im *im, double *out);
int smcpp_get_emission_probs_jac(smcpp_im *im, double *out);
/* getEmission() (include/inference_manager.h:72,166; src/inference_manager.cpp:392-407): the conditioned SFS after
 * incorporate_theta per hidden state, flattened row-major: [M x cols], cols = prod_p (a_p + 1)(n_p + 1);
 * jac [M*cols x nder] may be NULL. */
int smcpp_num_emission_cols(smcpp_im *im);
int smcpp_get_emission(smcpp_im *im, double *out, double *jac);
/* posterior decoding indices: argmax_m gamma[m, ell] for ell = 0..L (needs save_gamma) */
int smcpp_get_gamma_argmax(smcpp_im *im, int contig, int *out);

/* ---- multi-GPU ----------------------------------------------------------------------- */

/* Key dictionary shared by every rank (union of the ranks' smcpp_get_keys lists, lexicographic): fixes the layout
 * of the gamma_sums block of the packed buffer. */
int smcpp_set_global_keys(smcpp_im *im, int Kg, const int *gkeys);

/* Packed sufficient statistics of this rank's contigs, ready for one all-reduce(sum, fp64):
 * [ sum loglik | gamma0 (M) | xisum (M*M) | gamma_sums dense (K*M) ].  Returns the length via n_out when
 * buf == NULL.  dev != 0: buf is a device pointer (filled by one kernel on the engine's stream) else a host pointer.
 * dev == 1 returns after that kernel has finished; dev == 2 returns after the ENQUEUE: the caller consumes buf on the
 * engine's stream (smcpp_stream), e.g. an RCCL all-reduce ordered behind the pack kernel with no host wait in between. */
int smcpp_pack_stats(smcpp_im *im, double *buf, long *n_out, int dev);
/* Hand the all-reduced buffer back; Q() then evaluates on the global statistics. */
int smcpp_unpack_stats(smcpp_im *im, const double *buf, long n, int dev);

/* The same exchange issued by the engine itself through RCCL's C API on its own stream (no counterpart in the reference, which
 * sums over the contigs of one process: src/inference_manager.cpp:116-126, smcpp/_smcpp.pyx:303-308):
 *   smcpp_rccl_unique_id   rank 0 obtains the 128-byte ncclUniqueId (distribute it to the other ranks by any means);
 *   smcpp_rccl_init        every rank, after smcpp_set_global_keys: ncclCommInitRank on the manager's device;
 *   smcpp_rccl_exchange    after smcpp_estep: k_pack_stats -> ncclAllReduce(sum, f64, in place) -> the reduced sum of the
 *                          log-likelihoods into pinned host memory, all on the engine's stream; returns that sum;
 *   smcpp_rccl_unpack      hands the reduced statistics (still in the engine's device buffer) to Q();
 *   smcpp_rccl_fetch       (tests) a host copy of that buffer;  smcpp_rccl_destroy: ncclCommDestroy (also done by smcpp_destroy).
 * libpath: the RCCL library the process already uses (e.g. torch's lib/librccl.so), NULL or "" for "librccl.so.1"; it is resolved
 * with dlopen - the engine has no link-time dependency on RCCL. */
int smcpp_rccl_unique_id(const char *libpath, char *out128);
int smcpp_rccl_init(smcpp_im *im, const char *libpath, const char *id128, int rank, int world);
int smcpp_rccl_exchange(smcpp_im *im, double *loglik_sum);
int smcpp_rccl_unpack(smcpp_im *im);
int smcpp_rccl_fetch(smcpp_im *im, double *out, long n);
int smcpp_rccl_destroy(smcpp_im *im);

/* InferenceManager::debug (_smcpp.pxd:53): a public flag the reference declares to Cython; nothing in its C++ reads it. */
int smcpp_set_debug(smcpp_im *im, int on);
int smcpp_get_debug(smcpp_im *im);

/* ---- engine controls (no reference counterpart) ---------------------------------------------------------- */

/* Rows per chunk of the chunk-parallel chains (0 = automatic) and the chunk-boundary convergence tolerances. */
int smcpp_set_chunking(smcpp_im *im, int rows_per_chunk, double eps_alpha, double eps_beta);

/* Where the cold preparation of a one-population manager runs: 0 (default) = conditioned SFS, incorporate_theta and the
 * emission table on the device (smcpp_amd/csrc/prep_dev.hpp; the host only builds the O(pieces) rate function, pi and the
 * transition matrix), 1 = everything on the host (smcpp_amd/csrc/prep.hpp, rounds 1-3; also selected by SMCPP_PREP=host).
 * Results agree to the last bits of the exponentials; kept for the tests and as the baseline of bench.py --workload qgrad. */
int smcpp_set_prep_mode(smcpp_im *im, int host);

/* Extension (off by default): start the chunk-parallel chains of the next E-step from the converged chunk-boundary
 * vectors of the previous E-step of this manager instead of pi / the uniform vector.  In an EM or optimiser loop the
 * parameters move little between calls, so the re-run passes merge after a fraction of a chunk; the fixed-point
 * iteration and its convergence certificate are unchanged, results agree with a cold start within eps. */
int smcpp_set_warm_start(smcpp_im *im, int on);
/* Kernel-time breakdown of the last E-step in milliseconds:
 * [host_prep, chains_wall, forward, backward, stats, finalize, total_device, fwd_passes, bwd_passes]
 * (forward and backward overlap when the two chains run on separate streams; chains_wall is their union) */
int smcpp_last_timing(smcpp_im *im, double out[9]);
/* diagnostics: the chain kernel family in use (0 generic, 1 LDS-resident, 2 cooperative, 3 cooperative with streamed
 * operands, 4 lock-step on the matrix cores, 5 scans over the semiseparable structure of the transition matrix -
 * src/transition.cpp:176-254 - one position per step, no eigensystem; an E-step whose T lacks that structure runs the
 * dense kernels instead; 6 = family 5 with HYBRID rows: un-binned data, a row whose span exceeds a few positions is one
 * eigen-power step P d^s P^-1 inside the scan kernel - hmm.cpp:72-78,104-112 - instead of `span` scan steps) */
/* Host-only (no device needed): chunks per contig of the scan chains for `nslots` wavefront slots, cost[c] = positions (or cost
 * units) of contig c, rows[c] its row count; never more chunks than slots in total unless there are more contigs than slots, and
 * the longest chunk as short as the slot count allows (the reference parallelises over contigs only, inference_manager.cpp:89-94;
 * this is the engine's own decomposition, exported for the CPU tests). */
int smcpp_host_chunk_counts(int n_contigs, const long long *cost, const int *rows, long long nslots, long long floor_cost, int *out);
/* Host-only (no device needed, none touched): the plan of the chain phase a manager built from these arguments (n[p], na[p]: sample
 * sizes and distinguished lineages of the npop populations, as smcpp_create_onepop / _twopop take them) would resolve on a device
 * of `compute_units` compute units after smcpp_set_chunking(rows_per_chunk) (0: automatic), and the chunk lists it would cut.
 * Runs the host half of the construction - keys, rows, groups, the cut of long rows - and the same resolve and cut functions a
 * manager runs.  json (up to json_cap - 1 characters): {"plan": {..., "power_jumps": {...}}, "hybrid": {...} | null}
 * (the form of the hybrid rows' eigen-power step: tables in LDS, cold and hot eigen keys) as smcpp_describe prints it, with the
 * per-E-step entries ("light_passes_*", "halo_pass", "float_scans_in_stored_passes", "passes_launched", "power_jumps.run") as a first
 * E-step on a transition matrix of the reference's structure sets them.  chunks_fwd / chunks_bwd: up to chunk_cap chunks each in
 * smcpp_debug_chunks' five-int format.  lengths[3]: what the text and the two lists need (call with the caps 0 to size them). */
int smcpp_host_chain_plan(int npop, const int *n, const int *na, int n_contigs, const int *Ls, const int *const *obs,
                          int n_hs, const double *hs, int compute_units, int rows_per_chunk,
                          char *json, int json_cap, int *chunks_fwd, int *chunks_bwd, int chunk_cap, int *lengths);
/* Host-only (no device needed, none touched): the plan of the parameter phase - which preparation runs and why - that a manager in
 * this state resolves under the switches of the environment, as {"parameters": {...}} of smcpp_describe.  n: sample size of
 * population 1, pieces_plus_states: model pieces + hidden-state boundaries (what the device preparation's size limit is asked).
 * Writes at most json_cap - 1 characters; *length: what the text needs (call with json_cap 0 to size the buffer). */
int smcpp_host_param_plan(int npop, int have_raw, int force_host, int nder, int n, int pieces_plus_states, int have_global,
                          char *json, int json_cap, int *length);
/* Host-only (no device needed, none touched): the plan of the statistics phase and the layout it runs on, for a manager built from
 * the observation arguments of smcpp_host_chain_plan on a device of `compute_units` compute units, with save_gamma on or off.
 * structured_T != 0: the transition matrix has the reference's structure - the E-step runs on the scan chains where the chain plan
 * takes them, and generators of T exist.  json: {"statistics": {...}, "layout": {...}}: "statistics" as smcpp_describe prints it after
 * such an E-step; "layout": what the construction cut for the statistics kernels - rows of span 1 and span > 1, rows per slab, whether
 * the slab count was aimed at teams, the shares of the reductions, the blocks of the log-likelihood reduction, the eigen-power pieces
 * and, per list, its length and the 64-bit FNV-1a hash of its elements (little-endian, field by field); a slab list adds the rows its
 * slabs hold, its padding slabs and whether the slabs tile the sorted rows in order.  Writes at most json_cap - 1 characters;
 * *length: what the text needs (call with json_cap 0 to size the buffer). */
int smcpp_host_stats_plan(int npop, const int *n, const int *na, int n_contigs, const int *Ls, const int *const *obs, int n_hs,
                          const double *hs, int compute_units, int save_gamma, int structured_T, char *json, int json_cap, int *length);
int smcpp_chain_mode(smcpp_im *im);
/* diagnostics (host only): the chunk list of the scan chains as the last plan cut it - backward == 0: the forward chain's, else the
 * backward chain's (the two directions have lists of their own).  Writes up to `cap` chunks into out[5 * cap] as (contig, r0, r1, h0,
 * h1) and returns how many there are (call with cap = 0 to size the buffer); -1 on a NULL manager.  The chunk owns rows r0+1 .. r1 of
 * its contig, 1-based; a forward chunk enters through rows h0+1 .. h1 in float and h1+1 .. r0 in fp64 of its neighbour (h0 <= h1 <= r0),
 * a backward one through rows h0 .. h1+1 in float and h1 .. r1+1 in fp64 (h0 >= h1 >= r1); h0 == h1 == r0 (r1): no halo.  Rows are
 * the engine's own: where long rows are cut (plan "long_rows_cut") a caller's row of span s is ceil(s / 64) consecutive rows. */
int smcpp_debug_chunks(smcpp_im *im, int backward, int cap, int *out);
/* Every SMCPP_* environment switch of the engine is parsed ONCE per process (smcpp_amd/csrc/engine_options.hpp holds the one
 * table of them); smcpp_reload_options re-reads the environment (tests; never while an E-step runs).  smcpp_describe writes one
 * JSON object - the switches that are set and the plan `im` resolved (chain family, chunk counts, history passes, whether the
 * stored passes of the last E-step ran their scans in float; "q_route": whether the last smcpp_q was evaluated by the device
 * kernels, "device", by the host loops, "host", or not yet, "none"; "estep_redone": 1 when the last E-step ran twice - the scan
 * chains' attempt on a device-prepared emission table was abandoned because an entry is too small for `span` scan steps, and the
 * E-step redone on the dense kernels -, "estep_redone_why": the reason, "" otherwise; "estep_chain_family": the chain family the
 * last E-step ended on, -1 before the first; "scan_chains_refused": "", "transition structure" or "emission underflow", why a
 * manager planned for the scan chains ran its last E-step on the dense kernels) - and returns the length it needs; `im` may be NULL. */
void smcpp_reload_options(void);
int smcpp_describe(smcpp_im *im, char *buf, int cap);
/* Test hook of family 5: one position of both scan chains on nvec vectors: out_f = e o (T^T x), out_b = T (e o x); T is
 * [M][M] row-major, x / e / out_* are [nvec][M].  Returns 2 when T has no semiseparable structure (nothing is written). */
int smcpp_debug_ss_apply(int M, const double *T, int nvec, const double *x, const double *e, double *out_f, double *out_b);
/* ... the same position by the step of the stored passes with every scan in float (M <= 64; the M <= 32 form when M <= 32). */
int smcpp_debug_ss_apply_float_scans(int M, const double *T, int nvec, const double *x, const double *e, double *out_f, double *out_b);
/* ... and by every compiled form of the step (tests/test_gpu_ss_step.py), the production device functions on caller vectors:
 *   form 0  fp64 scans, 1 .. 16 states per lane (smcpp_debug_ss_apply)                                      M <= 1024
 *   form 1  float scans of the stored passes as the engine picks them: the two-row form at M <= 32          M <= 64
 *   form 2  float scans of the stored passes, full-width form also at M <= 32 (what SMCPP_SS_H32=0 runs)    M <= 64
 *   form 3  the all-float step of the light passes and of the float halo, 1 .. 16 states per lane           M <= 1024
 *   form 4  the all-float step, two-row form                                                                M <= 32
 *   form 5  power jumps: the tables of the P-th power of the operator with e[0] as the jump key's emission vector (every row of e
 *           should be that vector), then per vector out_f = A_f^k x, out_b = A_b^k x, A_f = diag(e) T^T, A_b = T diag(e);
 *           `power` = k = P (one jump) or 3 P (three jumps), P = 4, 8 or 16                                    M <= 64
 * `power` is 0 for the forms 0 .. 4.  A combination the engine never compiles is refused (1, smcpp_last_error) before any launch.
 * Returns 2 when T has no semiseparable structure, 3 when a power jump left anything but 0.0 on a padded state (M < 64). */
int smcpp_debug_ss_apply_form(int M, const double *T, int nvec, const double *x, const double *e, double *out_f, double *out_b, int form, int power);
/* Host phase of the last E-step in milliseconds: [cold preparation A6-A10 (0 when the parameters were still fresh or
 * came from smcpp_set_raw), eigensystems, layouts + staging + copy enqueue, whole host phase] */
int smcpp_last_host_timing(smcpp_im *im, double out[4]);
/* The HIP stream the engine launches on (a hipStream_t), for event timing by the caller. */
void *smcpp_stream(smcpp_im *im);
/* The HIP device the manager lives on (buffers handed to smcpp_pack_stats / smcpp_unpack_stats must live there). */
int smcpp_device(smcpp_im *im);

/* init_logger_cb (include/common.h, _smcpp.pxd:26, _smcpp.pyx:32-55): the engine's messages (level "DEBUG", "INFO",
 * "WARNING", ...) are handed to the binding, which forwards them to Python's logging; NULL = silent (the default). */
void smcpp_init_logger_cb(void (*cb)(const char *name, const char *level, const char *message));
/* init_cache (include/matrix_cache.h, _smcpp.pxd:87-88, src/matrix_cache.cpp:46-110): prefix of the on-disk store of the
 * n-only conditioned-SFS tables (exact-rational work: 0.35 s at n = 10, 0.9 s at n = 50 when computed); one file
 * `<path>.n<N>` per sample size, written atomically.  Empty / NULL = no store (tables live in the process only). */
int smcpp_init_cache(const char *path);
/* openmp.omp_set_num_threads (_smcpp.pyx:61-64): threads of the host-side preparation. */
void smcpp_set_num_threads(int k);

/* ---- pre-HMM data shaping on the device ------------------------------------------------ */

/* What `smc++ estimate` does to a contig before an inference manager sees it (smcpp/data_filter.py:166-203), as device kernels
 * over rows int32 [L][1 + 3 P] handed over by the caller (host memory; copied to HBM once):
 *   mode 0  thin_data(rows, thinning = p0, offset = p1)          smcpp/_estimation_tools.pyx:8-84
 *   mode 1  bin_observations(rows, w = p0), na[P] distinguished lineages per population   _estimation_tools.pyx:113-173
 *   mode 2  compress_repeated_obs(rows)                           smcpp/estimation_tools.py:51-60
 *   mode 3  Thin(p0) -> Bin(p1, na) -> Compress without leaving HBM (the pipeline of data_filter.py)
 * Bit-exact with the reference's code (goldens G23 / G11).  The result stays on the device (per calling thread): *rows_out = its
 * row count, *kernel_ms (optional) = the device time with the input resident in HBM; smcpp_dev_shape_fetch copies the rows out
 * (int32 [rows_out][ncol]).  smcpp_amd/data.py holds the host implementation of the same functions. */
int smcpp_dev_shape(int mode, long long L, int ncol, const int *rows, long long p0, long long p1, const long long *na,
                    long long *rows_out, double *kernel_ms);
int smcpp_dev_shape_fetch(int *out);

/* ---- host-only helpers (no device needed; used by the CPU test-suite) ------------------------------------ */

/* Test hook: 1 = evaluate the conditioned SFS term by term exactly as src/piecewise_constant_rate_function.cpp:214-334
 * and src/conditioned_sfs.cpp:42-83 write it (O(pieces^2 n^2), reproduces the compiled reference to 1e-15 relative);
 * 0 (default) = the factored O(pieces n^2) evaluation (same integrals through prefix / suffix sums over the pieces,
 * within 5e-16 absolute of the literal one on the emission table).  Returns the previous setting. */
int smcpp_host_set_csfs_direct(int on);

/* eigensystem(EigenSolver(A)) as TransitionBundle::update uses it (src/transition_bundle.cpp:22,
 * include/transition_bundle.h:9-30): P_r, Pinv_r [n x n], d_r [n], scale = max |d|, max |imag d|. */
int smcpp_host_eigensystem(int n, const double *A, double *P, double *Pinv, double *d, double *scale,
                           double *max_imag);
/* the same, computed by `threads` cooperating threads (smcpp_amd/csrc/nonsym_eig_team.hpp: bit-identical results); what the
 * engine uses for M >= 128 */
int smcpp_host_eigensystem_team(int n, const double *A, int threads, double *P, double *Pinv, double *d, double *scale,
                                double *max_imag);

/* One-population cold preparation without an engine instance:
 * model pieces (a, s)[Kp] + hidden states -> pi [M], T [M x M], E [K x M] for the given keys [K x 3]. */
int smcpp_host_prep_onepop(int n, int n_hs, const double *hs, double polarization_error, int Kp, const double *a,
                           const double *s, double theta, double rho, double alpha, int K, const int *keys,
                           double *pi, double *T, double *E);

/* The same with forward-mode derivative seeds da [Kp x nder] on the piece sizes: additionally returns the Jacobians
 * dpi [M x nder], dT [M*M x nder], dE [K*M x nder] (what the reference carries in its adouble type, common.h:22-25). */
int smcpp_host_prep_onepop_jac(int n, int n_hs, const double *hs, double polarization_error, int Kp, const double *a,
                               const double *da, int nder, const double *s, double theta, double rho, double alpha,
                               int K, const int *keys, double *pi, double *T, double *E, double *dpi, double *dT,
                               double *dE);

/* The same preparation with the conditioned SFS (A10), incorporate_theta and the emission table (A6) evaluated by the HIP
 * kernels of smcpp_amd/csrc/prep_dev.hpp - what smcpp_estep / smcpp_q run for one-population managers - instead of the host
 * routines (src/conditioned_sfs.cpp:13-148, src/inference_manager.cpp:389-482; pi and the transition matrix come from the
 * host either way).  mode 0: on the current HIP device; mode 1: the same kernel phases run serially on the host (no device
 * needed: CPU test-suite).  da / nder may be NULL / 0 (then dpi, dT, dE, dsfs are not written); sfs [M x 3(n+1)] and dsfs
 * [M*3(n+1) x nder] (the conditioned SFS per hidden state after incorporate_theta) may be NULL. */
int smcpp_dev_prep_onepop(int n, int n_hs, const double *hs, double polarization_error, int Kp, const double *a,
                          const double *da, int nder, const double *s, double theta, double rho, double alpha, int K,
                          const int *keys, int mode, double *pi, double *T, double *E, double *dpi, double *dT, double *dE,
                          double *sfs, double *dsfs);

/* Test hook (no device needed): Q's four terms (src/hmm.cpp:155-193) and their gradient jac [4 x nder] for statistics summed
 * over contigs - g0 [M], xi [M x M], gs [K x M] - computed by the phases of the device kernel (prep_dev.hpp: k_q_reduce) run
 * serially on the host, from the emulated device preparation and the O(M) generator planes of the transition matrix: the data
 * path smcpp_q takes on the GPU for one-population managers. */
int smcpp_dev_q_emulate(int n, int n_hs, const double *hs, double polarization_error, int Kp, const double *a, const double *da,
                        int nder, const double *s, double theta, double rho, double alpha, int K, const int *keys,
                        const double *g0, const double *xi, const double *gs, double *val, double *jac);

/* Test hook (no device needed): the transition matrix T [M x M] of a one-population model (pieces a, s; seeds da [Kp x nder],
 * nder >= 1; hidden states hs [n_hs], M = n_hs - 1), its dense Jacobian dT [M x M x nder] as the engine expands it from the O(M)
 * generator planes, and the four COEFFICIENT PLANES [nder x M] the vector form of the score track (SMCPP_SCORE_FORM=vectors)
 * contracts with instead of dT.  With c0 = 1e-5 / (M + 1), entry by entry
 *     dT_d(i, j) = cL_d(j) T(i, j)  (i > j),   (cP_d(i) + cW_d(j)) (T(i, j) - c0)  (i < j),   cD_d(j) T(j, j)  (i == j),
 * except above the diagonal where the raw entry lies below the 1e-20 floor (dT is zero there, the planes keep the raw product).
 * Fails when the generators need the pairwise fallback (cumulative hazard beyond 575). */
int smcpp_host_score_planes(int Kp, const double *a, const double *da, int nder, const double *s, int n_hs, const double *hs,
                            double rho, double *T, double *dT, double *cD, double *cL, double *cW, double *cP);

/* PyRateFunction.R / average_coal_times (smcpp/_smcpp.pyx:370-389): cumulative hazard R at t[0..nt) for the model
 * pieces (a, s) and, when n_hs >= 2, E[T | hs_i <= T < hs_{i+1}] for the n_hs-1 intervals. */
int smcpp_host_rate_function(int Kp, const double *a, const double *s, int n_hs, const double *hs, int nt,
                             const double *t, double *R_out, double *avg_ct_out);

/* The same with derivative seeds (PyRateFunction on a model with differentiable pieces): dR_out [nt x nder],
 * davg_ct_out [(n_hs-1) x nder]. */
int smcpp_host_rate_function_jac(int Kp, const double *a, const double *da, int nder, const double *s, int n_hs,
                                 const double *hs, int nt, const double *t, double *R_out, double *dR_out,
                                 double *avg_ct_out, double *davg_ct_out);

/* PyRateFunction.random_coal_times (smcpp/_smcpp.pyx:391-399, piecewise_constant_rate_function.cpp:337-368): K
 * coalescence times conditioned on [t1, t2), one std::mt19937 per draw seeded with seeds[i]; returns t and R(t). */
int smcpp_host_random_coal_times(int Kp, const double *a, const double *s, double t1, double t2, int K,
                                 const unsigned long long *seeds, double *t_out, double *R_out);

/* raw_sfs (smcpp/_smcpp.pyx:401-412, sfs_cython inference_manager.cpp:492-504): the 3 x (n+1) conditioned SFS of the
 * single hidden state [t1, t2) before incorporate_theta; dsfs [3*(n+1) x nder] may be NULL when nder == 0. */
int smcpp_host_raw_sfs(int n, int Kp, const double *a, const double *da, int nder, const double *s, double t1,
                       double t2, int below_only, double *sfs, double *dsfs);

/* TwoPopInferenceManager::setParams (src/inference_manager.cpp:542-550, smcpp/_smcpp.pyx:353-368): the distinguished
 * model (pi, transition, average coalescence times), the two per-population models and the split time for the joint
 * CSFS.  d* are derivative seeds [K x nder] (NULL = zero) sharing one set of nder directions (`model.dlist`). */
int smcpp_set_params_twopop(smcpp_im *im, int Kd, const double *ad, const double *sd, const double *dad, int K1,
                            const double *a1, const double *s1, const double *da1, int K2, const double *a2,
                            const double *s2, const double *da2, double split, int nder);

/* joint_csfs (smcpp/_smcpp.pyx:416-437; JointCSFS src/jcsfs.cpp:219-420): per hidden state the tensor
 * [(a1+1) x (n1+1) x (a2+1) x (n2+1)], out [(n_hs-1) x that], Kmc Monte-Carlo draws for the averaged Moran
 * transition below the split (the reference's default is 10).  With nder > 0, da1 / da2 [K x nder] seed the piece
 * sizes (NULL = zero) and dout [size x nder] receives the Jacobian. */
int smcpp_host_joint_csfs(int n1, int n2, int a1, int a2, int n_hs, const double *hs, int K1, const double *pa1,
                          const double *ps1, const double *da1, int K2, const double *pa2, const double *ps2,
                          const double *da2, int nder, double split, int Kmc, double *out, double *dout);

/* Whole two-population cold preparation without an engine instance: pi [M], T [M x M], E [K x M] for keys [K x 6]. */
int smcpp_host_prep_twopop(int n1, int n2, int a1, int a2, int n_hs, const double *hs, double polarization_error,
                           int Kd, const double *ad, const double *sd, int K1, const double *pa1, const double *ps1,
                           int K2, const double *pa2, const double *ps2, double split, double theta, double rho,
                           double alpha, int K, const int *keys, double *pi, double *T, double *E);

/* ---- posterior products on the device (no reference counterpart; smcpp_amd/csrc/posterior_dev.hpp) ------------------- */

/* Products of the per-row posteriors of the LAST E-step, which must have run with save_gamma, computed by kernels that read the rows
 * where they lie.  Contig `contig` has L caller's rows with spans s_1 .. s_L; gamma is the [M x (L + 1)] matrix smcpp_get_gamma
 * returns and p[:, l] = gamma[:, l] / sum_m gamma[m, l].  A column selection is range(start, stop, step) over 0 .. L, of
 * ncols = ceil((stop - start) / step) columns.  All pointers are host pointers; output pointers that are NULL are skipped.  Each
 * call fails before anything is launched when no E-step has run, the last one ran without save_gamma, the contig index is out of
 * range, start < 0, stop > L + 1, start >= stop, step < 1, window_bp < 1, nq outside 0 .. 8, a level outside (0, 1), or a weight
 * that is not finite.
 *
 * smcpp_posterior_columns: out [M x ncols] row-major, doubles or (f32 != 0) floats: p if normalize != 0, else gamma (a copy:
 * bit for bit what smcpp_get_gamma returns); colsum [ncols] the column sums (states added in ascending order). */
int smcpp_posterior_columns(smcpp_im *im, int contig, long long start, long long stop, long long step,
                            int normalize, int f32, void *out, double *colsum /* may be NULL */);
/* smcpp_posterior_summary: per selected column, without forming the matrix: colsum, argmax (the first maximum, as
 * smcpp_get_gamma_argmax), mean = sum_m weights[m] p[m, l] (skipped when weights is NULL), and for each of the nq levels q[k]
 * qstate[k x ncols] = min{m : sum_{i <= m} p[i, l] >= q[k]} (running sum in ascending order). */
int smcpp_posterior_summary(smcpp_im *im, int contig, long long start, long long stop, long long step,
                            const double *weights /* [M] or NULL */, int nq, const double *q,
                            double *colsum, int *argmax, double *mean, int *qstate /* [nq x ncols] */);
/* smcpp_posterior_windows: the average of p over windows of window_bp base pairs.  With P_l = s_1 + .. + s_l row l >= 1 covers
 * base pairs [P_{l-1}, P_l); window w covers [w W, min((w + 1) W, P_L)); out[:, w] = sum_l overlap(l, w) p[:, l] / (base pairs of
 * the window that are covered), rows added in ascending order.  Column 0 of gamma takes no part.  *n_windows = ceil(P_L / W);
 * out [M x n_windows] row-major. */
int smcpp_posterior_windows(smcpp_im *im, int contig, long long window_bp, long long *n_windows,
                            double *out /* [M x n_windows]; NULL: only n_windows is written */);

/* ---- posterior transition products on the device (no reference counterpart; smcpp_amd/csrc/posterior_trans_dev.hpp) --- */

/* Where the hidden state changes along a contig, from the vectors the LAST E-step stored (it must have run with save_gamma, and
 * the parameters must not have been set again since).  Row l of contig `contig` has span s_l and key k_l and covers positions
 * P_{l-1} + 1 .. P_l.  For a position p of row l, with x_{p-1} the forward vector before it, y_p the backward vector after it and
 * e = E[k_l] the row's emission vector,
 *     xi_p(i, j) = x_{p-1}(i) T(i, j) e(j) y_p(j) / Z_p,        Z_p = sum_ij of the numerator,
 *     stay[l] = sum_{p in row l} sum_i xi_p(i, i),
 *     up[l]   = sum_{p in row l} sum_{i<j} xi_p(i, j)           (to a higher index = older state),
 *     down[l] = sum_{p in row l} sum_{i>j} xi_p(i, j),
 * so stay + up + down = s_l, s_l - stay[l] is the expected number of state changes in the row, and the sums over the rows of a
 * contig are the trace and the strict upper / lower triangle sums of its xisum.  Column 0, which no transition enters, holds
 * (0, 0, 0).  x and y are scale free: they start from the stored float alpha at the row's start and the stored beta at its end and
 * are advanced through the row's interior by the O(M) scan steps of the semiseparable transition matrix; where the plan cut long
 * rows, the pieces of a caller's row are added up on the device.  Results do not depend on the launch shape or on call order.
 * Each call fails before anything is launched when no E-step has run, the last one ran without save_gamma, the contig index is out
 * of range, start < 0, stop > L + 1, start >= stop, step < 1, window_bp < 1, the parameters were set again after the last E-step,
 * or the transition matrix lacks the semiseparable structure (smcpp_set_raw with an arbitrary matrix).
 *
 * smcpp_posterior_transitions: the three values on the column selection range(start, stop, step) over 0 .. L. */
int smcpp_posterior_transitions(smcpp_im *im, int contig, long long start, long long stop, long long step,
                                double *stay, double *up, double *down /* each [ncols] or NULL */);
/* smcpp_posterior_transition_windows: expected counts per window of window_bp base pairs, a row apportioned uniformly over its
 * base pairs: out[x, w] = sum_l overlap(l, w) / s_l * x[l] for x = stay, up, down, rows added in ascending order (windows as in
 * smcpp_posterior_windows).  The three values of a window sum to its covered base pairs.  *n_windows = ceil(P_L / W). */
int smcpp_posterior_transition_windows(smcpp_im *im, int contig, long long window_bp, long long *n_windows,
                                       double *out /* [3 x n_windows] row-major; NULL: only n_windows */);

/* ---- posterior paths (posterior_paths_dev.hpp): joint draws of the hidden-state path of contig c from the posterior of the last
 * save_gamma E-step, by forward filtering and backward sampling.  Conventions as for the transition products: caller's rows
 * l = 1 .. L with spans s_l, P_l = s_1 + .. + s_l, positions 0 .. N with N = P_L; position 0 is column 0, row l covers positions
 * P_{l-1} + 1 .. P_l; a_0 = pi and a_p = e_p o (T^T a_{p-1}), renormalised freely.  Path k:
 *     x_N is drawn with weights w_i = a_N(i);  for q = N - 1 .. 0, x_q given x_{q+1} = j is drawn with weights w_i = a_q(i) T(i, j).
 * Every draw is an inverse CDF in ASCENDING state order:  C_i = w_0 + .. + w_i,  x = min{ i : C_i > u C_{M-1} }, clamped to M - 1.
 * The uniform of the draw of x_q of path k comes from Philox4x32-10 (round multipliers 0xD2511F53, 0xCD9E8D57; key increments
 * 0x9E3779B9, 0xBB67AE85) with key = (seed & 0xffffffff, seed >> 32) and counter = (q & 0xffffffff, q >> 32, k, contig):
 *     u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53    from output words w0, w1.
 * Known answers (counter / key -> output):
 *     0 0 0 0 / 0 0                                              -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8   (u = 0.39904647231489565)
 *     ffffffff x 4 / ffffffff x 2                                -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344 / a4093822 299f31d0    -> d16cfe09 94fdcceb 5001e420 24126ea1
 * Path k of contig c under `seed` is therefore a pure function of the stored vectors, seed, c and k: it does not depend on how many
 * paths a call asks for, on the window or selection it returns, on how paths are grouped onto wavefronts (SMCPP_PATH_BATCH) or on
 * what ran before, and a caller can reproduce it on the host from smcpp_get_pi / _transition / _emission_probs.  The device takes
 * a_q from what the E-step stored: the float alpha at the row's start (a_0: the stored column 0), advanced through the row's
 * interior by the O(M) scan step and kept as floats, so its CDF agrees with the float64 one to the accuracy of the per-row
 * posterior (bar 2e-5; tests/test_gpu_posterior_paths.py holds every draw to it); T(i, j) is the manager's transition matrix in fp64; beta is not used.
 * Preconditions are those of smcpp_posterior_transitions, and: npaths >= 1, path0 >= 0, path0 + npaths <= 2^31,
 * 0 <= pos0 < pos1 <= P_L + 1, at most 2^31 - 1 output elements per array and call (also npaths x engine rows), at most 1 GiB of
 * scratch.  Every failure happens before anything is launched.
 *
 * smcpp_posterior_sample_rows: per caller's row of the selection range(start, stop, step) over 0 .. L the state at the row's last
 * position and the number of positions p of the row with x_{p-1} < x_p (up) / x_{p-1} > x_p (down); column 0: the state at
 * position 0 and (0, 0). */
int smcpp_posterior_sample_rows(smcpp_im *im, int contig, unsigned long long seed, long long path0, long long npaths,
                                long long start, long long stop, long long step,
                                int *state, int *up, int *down /* each [npaths x ncols] row-major or NULL */);
/* smcpp_posterior_sample_positions: the states at positions pos0 .. pos1 - 1 of 0 .. P_L. */
int smcpp_posterior_sample_positions(smcpp_im *im, int contig, unsigned long long seed, long long path0, long long npaths,
                                     long long pos0, long long pos1, int *out /* [npaths x (pos1 - pos0)] row-major */);

/* ---- posterior positions (posterior_pos_dev.hpp): the posterior of SINGLE positions of contig c, as a distribution.  Conventions
 * as for the path sampler: caller's rows l = 1 .. L with spans s_l, P_l = s_1 + .. + s_l, positions 0 .. N with N = P_L; position 0
 * is column 0, row l covers positions P_{l-1} + 1 .. P_l;
 *     a_0 = pi, a_p = e_p o (T^T a_{p-1});   b_N = 1, b_{p-1} = T (e_p o b_p);   gamma_p(i) = a_p(i) b_p(i) / sum_m a_p(m) b_p(m).
 * gamma_0 is column 0 of smcpp_posterior_columns(normalize = 1), and the marginal of the one position of a row with s_l = 1 is that
 * row's column of it, bit for bit.  Inside longer rows the device walks from what the E-step stored - the float alpha at the row's
 * start (its entries at the 1e-10 floor restored from the row before where that row is one position), beta at its end, the O(M)
 * scan steps in between, a_p kept as floats - so gamma_p agrees with the float64 one to the accuracy
 * of the per-row posterior (bar 2e-5; tests/test_gpu_posterior_positions.py holds every position to it).  A grid is
 * range(pos0, pos1, step) over 0 .. N, npos = ceil((pos1 - pos0) / step) positions.  A value is a pure function of the stored vectors
 * and the position: not of the grid, the launch shape, the call order or what ran before.
 * Preconditions are those of smcpp_posterior_transitions, and: 0 <= pos0 < pos1 <= N + 1, step >= 1, window_bp >= 1, 0 <= nq <= 8,
 * levels in (0, 1), finite weights, at most 2^31 - 1 output elements per array, at most 1 GiB of scratch (the checkpoints of the
 * longest walked row; the segment sums of the exact windows).  Every failure happens before anything is launched.
 *
 * smcpp_posterior_positions: gamma_p of every grid position. */
int smcpp_posterior_positions(smcpp_im *im, int contig, long long pos0, long long pos1, long long step,
                              double *out /* [M x npos] row-major */);
/* smcpp_posterior_position_summary: per grid position, without storing the column: argmax = the lowest state that attains the
 * maximum; mean = sum_m weights[m] gamma_p(m) (skipped when weights is NULL); per level q_k of nq <= 8:
 * qstate = min{ m : sum_{i <= m} gamma_p(i) >= q_k }, clamped to M - 1. */
int smcpp_posterior_position_summary(smcpp_im *im, int contig, long long pos0, long long pos1, long long step,
                                     const double *weights /* [M] or NULL */, int nq, const double *q /* [nq] */,
                                     int *argmax /* [npos] or NULL */, double *mean /* [npos] or NULL */,
                                     int *qstate /* [nq x npos] row-major or NULL */);
/* smcpp_posterior_windows_exact: windows as in smcpp_posterior_windows (base pair b is position b + 1), but exact on long rows:
 *     out[:, w] = (1 / covered_w) sum_{p - 1 in [w W, min((w + 1) W, N))} gamma_p.
 * A row inside one window contributes s_l p[:, l] from the stored per-row posterior; a row that k >= 1 window boundaries cut is walked
 * and contributes its k + 1 segment sums.  The terms of a window are added in ascending position order. */
int smcpp_posterior_windows_exact(smcpp_im *im, int contig, long long window_bp, long long *n_windows,
                                  double *out /* [M x n_windows] row-major; NULL: only n_windows */);

/* ---- log-likelihood track (loglik_track_dev.hpp): WHERE along contig c the log-likelihood of the last E-step comes from.  The
 * reference keeps one number per row, HMM::log_c (hmm.h; filled by HMM::forward_backward and only ever summed, HMM::loglik); the
 * three entries extend that interface.  Conventions as for the posterior positions: caller's rows l = 1 .. L with spans s_l,
 * P_l = s_1 + .. + s_l, positions 0 .. N with N = P_L; position 0 carries no observation.
 *     l(p) = log P(o_1 .. o_p),   l(0) = 0,   l(P_l) = sum_{r <= l} log c_r  (the engine's own per-row values; a caller's row the
 *     engine cut into pieces is the sum of its pieces), so l(N) is what smcpp_loglik reports for the contig.
 * Inside an engine row r of span s that starts behind position p0, with e the emission vector of its key: x_0 = the stored float
 * forward vector in front of the row, normalised; x_q ~ e o (T^T x_{q-1}); z_q = the sum of e o (T^T x_{q-1}) for normalised
 * x_{q-1}; A_q = sum_{t <= q} log z_t (fp64) and
 *     l(p0 + q) = l(p0) + log c_r  A_q / A_s:
 * the walk splits the row's stored log c in the proportions of its own running sum, so l is continuous at row ends, does not
 * increase wherever log c_r <= 0, and windows add up to the contig's log-likelihood whatever the float start vector did to A_s.
 * A value is a pure function of the stored vectors and the position: not of the grid, the launch shape (SMCPP_LL_WAVES), the call
 * order or what ran before.  smcpp_describe reports "ll_items" (engine rows walked), "ll_waves" and "ll_walk_worst_ratio", the
 * worst |A_s / log c_r - 1| of the last call.
 * Preconditions: an E-step has been run and the parameters have not been set since - a PLAIN one is enough (save_gamma is not
 * needed: every E-step plan leaves the forward vector and log c of every engine row in memory), and the posterior buffers are
 * neither needed nor disturbed; _positions and _windows also need a transition matrix with the model's semiseparable structure
 * (as smcpp_posterior_transitions); a valid selection / grid, window_bp >= 1, at most 2^31 - 1 output elements.  Every failure
 * happens before anything is launched and leaves the manager usable.  out == NULL runs the checks alone.
 *
 * smcpp_loglik_rows (extends HMM::log_c, hmm.h): log c of the caller's rows of the selection range(start, stop, step) over
 * 0 .. L, the selection rule of smcpp_posterior_summary; row 0 gives 0, as log_c[0] does in the reference. */
int smcpp_loglik_rows(smcpp_im *im, int contig, long long start, long long stop, long long step, double *out /* [ncols] */);
/* smcpp_loglik_positions (extends HMM::log_c, hmm.h, below the row): l on the grid pos0, pos0 + step, .. < pos1 of 0 .. N,
 * 0 <= pos0 < pos1 <= N + 1. */
int smcpp_loglik_positions(smcpp_im *im, int contig, long long pos0, long long pos1, long long step, double *out /* [npos] */);
/* smcpp_loglik_windows (extends HMM::log_c, hmm.h, to windows of base pairs): out[w] = l(min((w + 1) W, N)) - l(w W) for
 * w = 0 .. ceil(N / W) - 1; the windows sum to the contig's log-likelihood. */
int smcpp_loglik_windows(smcpp_im *im, int contig, long long window_bp, long long *n_windows,
                         double *out /* [n_windows]; NULL: only n_windows */);

/* ---- score track (score_track_dev.hpp): WHERE along contig c the derivative of the log-likelihood with respect to the model comes
 * from.  The reference knows that derivative only as one vector per manager, the Jacobian of InferenceManager::Q
 * (src/inference_manager.cpp:116-126; at the E-step's own parameters it is the gradient of the log-likelihood, by Fisher's
 * identity); the two entries split it along the contig.  All values are the arrays the getters return, floors included (a floored
 * entry has a zero Jacobian): with nder >= 1 directions from the last smcpp_set_params / _twopop, elementwise
 *     G_pi,d = dpi_d / pi,     G_T,d = dT_d / T,     G_E,d[k] = dE_d[k] / E[k].
 * Conventions as for smcpp_posterior_transitions: for position p of row l, with key k_l,
 *     xi_p(i, j) = x_{p-1}(i) T(i, j) e(j) y_p(j) / Z_p,     gamma_p(j) = sum_i xi_p(i, j),
 *     u_p[d] = sum_ij xi_p(i, j) G_T,d(i, j)            (transition part)
 *            + sum_j gamma_p(j) G_E,d[k_l](j)            (emission part),
 *     u_0[d] = sum_m gamma_0(m) G_pi,d(m)                (initial part, position 0 only),
 * and score_rows[d, l] = sum_{p in row l} u_p[d]; column 0 holds u_0.  gamma_0 is the NORMALISED column 0 (column 0 of
 * smcpp_posterior_columns(normalize = 1)), so that the sum of a contig's columns is the gradient of its log-likelihood.  Summed
 * over a contig's columns and over contigs the emission part is rows 1 + 2 and the transition part row 3 of smcpp_q's Jacobian on
 * the same E-step; row 0 of that Jacobian is sum_c m_c u_0,c with m_c the mass of contig c's column 0 AS STORED - the reference's
 * gamma[:, 0] = alpha_0 o beta_0 with beta_0 / sum beta_0 (src/hmm.cpp:150), which Q weighs log pi with and which does not sum to one.
 * x and y are those of the transition products: the stored float alpha at the row's start, the stored beta at its end, the O(M)
 * scan steps in between; where the plan cut long rows the pieces of a caller's row are added up on the device in ascending order.
 * A value is a pure function of the stored vectors, the tables and the row: not of the selection, the launch shape
 * (SMCPP_SCORE_WAVES), the call order or what ran before; the posterior buffers, the statistics and the loglik track are neither
 * needed beyond the stored vectors nor disturbed.  The Jacobian of a device-prepared emission table is copied out without
 * replacing the host's table, so a later smcpp_q KEEPS its device route after a score call ("q_route" stays what it was).
 * smcpp_describe reports "score_items" (engine rows walked), "score_waves", "score_park" ("lds" / "global": where a block's vectors
 * wait) and "score_form" ("matrix" / "vectors": the form of the last score call).
 * The row walk has two forms, chosen by the switch SMCPP_SCORE_FORM, which is read at EVERY call (one manager answers in both
 * without a new E-step):
 *     matrix  (unset)  one column of the M x M accumulator sum_p x_{p-1}(i) w_p(j) / Z_p per lane, contracted with the dense dT once
 *                      per row (score_track_dev.hpp); one state per lane, M <= 64.
 *     vectors          four O(M) accumulators per row against the coefficient planes of the transition Jacobian
 *                      (score_vec_dev.hpp; the dense dT is not expanded); one to four states per lane, M <= 256.  It needs the
 *                      generator planes of the transition Jacobian, which one-population models prepared on the device have: it
 *                      refuses SMCPP_PREP=host, two-population managers and a transition matrix that took the pairwise fallback.
 *                      Above the diagonal an entry below the 1e-20 floor keeps its raw derivative where the dense Jacobian has
 *                      zero: less than 1e-20 / c0 |dT / T| per position, c0 = 1e-5 / (M + 1).
 * Each call fails before anything is launched, and leaves the manager usable, when no E-step has run, the last one ran without
 * save_gamma, the contig index is out of range, the parameters were set again since the last E-step, they carry no derivative
 * seeds (nder = 0, or smcpp_set_raw), the transition matrix lacks the semiseparable structure, there are more than 64 hidden states
 * (the matrix form keeps one column of the M x M accumulator per lane) or more than 256 (the vectors
 * form), SMCPP_SCORE_FORM holds another word, the selection is bad (start < 0, stop > L + 1, start >= stop,
 * step < 1) or window_bp < 1, an output would exceed 2^31 - 1 elements or the scratch 1 GiB.
 *
 * smcpp_score_rows: the column selection range(start, stop, step) over 0 .. L, the selection rule of smcpp_posterior_summary.
 * parts != 0: the three parts; parts == 0: their sum (initial + emission) + transition, in that order. */
int smcpp_score_rows(smcpp_im *im, int contig, long long start, long long stop, long long step, int parts,
                     double *out /* parts == 0: [nder x ncols]; parts != 0: [3 x nder x ncols] initial, emission, transition; NULL: the checks alone */);
/* smcpp_score_windows: per window of window_bp base pairs (windows as in smcpp_posterior_transition_windows), a row apportioned
 * uniformly over its base pairs: out[d, w] = sum_l overlap(l, w) / s_l * score_rows[d, l], rows added in ascending order; column 0's
 * initial part goes to window 0, in front of the rows.  *n_windows = ceil(P_L / W). */
int smcpp_score_windows(smcpp_im *im, int contig, long long window_bp, long long *n_windows,
                        double *out /* [nder x n_windows] row-major; NULL: only n_windows */);
/* smcpp_score_windows_exact: the shape and the windows of smcpp_score_windows, but EXACT on the engine rows that a window boundary
 * cuts strictly inside (position p >= 1 of the contig lies in window (p - 1) / W): such a row gives every window the sum of u_p over
 * the positions that lie in it,
 *     out[d, w] = [w == 0] u_0[d] + sum_{p : (p - 1) / W == w} u_p[d],
 * what smcpp_score_rows would give on the same data with every row expanded into rows of span 1, added up by window.  Rows that lie
 * wholly inside a window come from the row walk as before; a cut row is walked a second time by k_score_segments_vec
 * (score_seg_dev.hpp), which closes a segment at every window boundary; then one wavefront per window adds the rows and segments
 * that overlap it in ascending position order, compensated.  Values are pure functions of the stored vectors, the tables and W.
 * The VECTORS form only (M <= 256, under that form's requirements above): with SMCPP_SCORE_FORM unset or "matrix" the call is
 * refused - set SMCPP_SCORE_FORM=vectors.  SMCPP_SCORE_WAVES caps the wavefronts of the segment walk as well.  Refused besides, as
 * everything above before any launch: 3 x nder x (segments of cut rows) beyond 2^31 - 1 elements, or the parts per engine row and
 * per segment with one wavefront's scratch beyond 1 GiB.  smcpp_describe reports "score_exact_items" (the rows a boundary cut),
 * "score_exact_segments" and "score_exact_waves" (0: no row was cut and the segment walk was not launched) of the last exact call. */
int smcpp_score_windows_exact(smcpp_im *im, int contig, long long window_bp, long long *n_windows,
                              double *out /* [nder x n_windows] row-major; NULL: only n_windows */);

/* ---- simulation (simulate_dev.hpp): draws of (hidden path, observations) from the model the manager holds - the process whose
 * marginal likelihood the E-step computes.  A simulated contig has positions 1 .. N; position 0 is column 0 and carries no
 * observation:
 *     x_0 ~ pi;   for p = 1 .. N:   x_p ~ T(x_{p-1}, .),   o_p ~ Ebar(. | x_p).
 * Observations are indices into an ALPHABET: alpha_keys[n_alpha], distinct key indices of the manager (rows of
 * smcpp_get_emission_probs, the order of smcpp_get_keys), of which `quiet` (a key index that occurs in alpha_keys) is the
 * monomorphic observation.  Ebar(k | m) = E[k][m] / sum_{k' in A} E[k'][m]: the draw always normalises over the alphabet.
 *
 * The walk is by EVENTS, not by positions.  With i = x_p and s_i = T(i, i) Ebar(q | i), a QUIET position keeps the state and emits q.
 * Event e = 0, 1, .. starts at (p, i) and takes three uniforms u_0, u_1, u_2:
 *     u_0  the quiet run  G = floor(log(1 - u_0) / log s_i)  (P(G >= g) = s_i^g), clamped to N - p; s_i = 0: G = 0; s_i >= 1:
 *          G = N - p.  If p + G >= N the contig is finished (the event leaves no record).
 *     u_1  the state j at the LOUD position p + G + 1, weights W_j = T(i, j) for j != i and W_i = T(i, i) (1 - Ebar(q | i)).
 *     u_2  the key at that position, weights E[k][j] in alphabet order, the weight of q being 0 when j = i.
 * Both draws are inverse CDFs in ASCENDING order, x = min{ j : C_j > u C_last }, clamped to the last index (the rule of the path
 * sampler above).  x_0 is drawn in the same way from pi with the spare uniform u_3 of event 0.  u_t of event e is pp_uniform of
 * the path sampler: Philox4x32-10 with counter = (q & 0xffffffff, q >> 32, replicate, contig), q = 4 e + t, and
 * key = (seed & 0xffffffff, (seed >> 32) ^ 0x53494D55) - a seed shared with smcpp_posterior_sample_* does not reuse its uniforms -
 * and u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53.  Contig c of the call has counter word contig0 + c, replicate r of the call
 * rep0 + r.  A replicate of a contig under a seed is therefore a pure function of (pi, T, E, A, q, N, seed, contig, replicate): not
 * of how many replicates a call asks for, of how they sit on wavefronts, of `cap`, or of what ran before.
 *
 * Arithmetic: fp64 throughout.  Per state the host adds the alphabet's mass in alphabet order, forms s_i and log s_i with the
 * host's log, and 1 - Ebar(q | i) as the sum over the alphabet WITHOUT q divided by the mass (no cancellation); the device takes
 * log(1 - u_0) (1 - u_0 is exact) and the two CDFs (lane-local prefix sums plus a wave scan: not the sequential order).
 *
 * A call draws at most `cap` events per replicate.  Outputs, all [n_contigs x nreps] row-major in front: x0 = x_0 where this call
 * drew it, else -1; n_events = loud positions written by this call; pos (int64), state, key (int32) [.. x cap]: position, state and
 * ALPHABET index of each loud position, ascending (entries beyond n_events are unspecified); resume_out [.. x 3] =
 * (next event index, position reached, state there).  A replicate is finished when its position equals N.  resume_in (NULL: every
 * replicate starts at (0, 0, -1) = nothing drawn yet) takes what an earlier call returned in resume_out: a run continued through
 * any sequence of caps gives the bits of an uncapped one.
 * The call fails before anything is launched when: the parameters are not set; a length < 1, nreps < 1 or cap < 1; an alphabet
 * index is out of range or given twice; quiet is not in the alphabet; a state gives the alphabet no mass; rep0 < 0 or
 * rep0 + nreps > 2^31; contig0 < 0 or contig0 + n_contigs > 2^32; n_contigs x nreps x cap > 2^31 - 1; a resume state that no call
 * can have returned.  With every output pointer NULL the call runs these checks alone.  The parameters are prepared if need be (as
 * smcpp_q does); no E-step is needed, and none is disturbed. */
int smcpp_simulate(smcpp_im *im, int n_contigs, const long long *lengths, int n_alpha, const int *alpha_keys, int quiet,
                   unsigned long long seed, long long contig0, long long rep0, long long nreps, long long cap,
                   const long long *resume_in /* [n_contigs x nreps x 3] or NULL */, int *x0, long long *n_events,
                   long long *pos, int *state, int *key, long long *resume_out);

#ifdef __cplusplus
}
#endif
#endif
