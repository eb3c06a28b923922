/*
 * vireo_hip.h -- C ABI of libvireo_hip.so: the MI355X (gfx950) implementation of the
 * vireoSNP variational-EM hot path.
 *
 * The reference (vireoSNP 0.5.9, pure Python) has no FFI layer; its boundary for this
 * path is the Python API (class Vireo, class BinomMixtureVB, vireo_wrap).  This header is
 * what a ctypes binding of that API calls.  Each entry point names the reference
 * interface (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; vrx_last_error() gives the
 *     thread-local message of the last failing call.
 *   - all pointers are HOST pointers to caller-owned memory; the library copies in/out
 *     and retains nothing across calls (device state lives behind the opaque handles).
 *   - dense arrays are C-contiguous float64 in the reference's own shapes:
 *       ID_prob (n_cell, n_donor)   GT_prob (n_var, n_donor, n_gt)
 *       beta_mu/beta_sum (theta_rows, n_gt) for Vireo [theta_rows = n_var in ASE mode
 *       else 1], (n_var, n_donor) for BinomMixtureVB.
 *   - one host thread per handle; distinct handles may be driven concurrently.
 *   - a model's VISIBLE STATE is: its state arrays (ID_prob, GT_prob, beta_mu, beta_sum; per
 *     restart in a batch), the priors as last set, logLik_ID on the device, the content of the
 *     snapshot slot (if anything was saved) and of the two staging buffers.  The results of a
 *     call -- what it returns and the visible state it leaves -- depend on the visible state
 *     alone, bit for bit, never on which calls came before: whatever the library defers or
 *     caches between calls is invisible here.  A fresh model of the same problem and
 *     configuration that is given the visible state (set_prior, set_state, set_loglik,
 *     snapshot, stage_raw) continues exactly as the old one would.
 *   - logLik_ID on the device is defined by VRX_STEP_ID, VRX_STEP_LOGLIK, vrx_model_fit and
 *     vrx_model_run_iters (their last iteration's, on every kernel path) and by
 *     vrx_model_set_loglik; it is all zeros in a new model.  The other calls leave it alone.
 *   - vrx_model_get_elbo_parts is defined only straight after a call that computed an ELBO
 *     (VRX_STEP_ELBO, vrx_model_fit, vrx_model_run_iters): the parts of the last ELBO that call
 *     computed.  No other successful call may come between.
 *   - a refused call (any error return of an argument check: a restore with nothing saved, a
 *     staged upload before vrx_model_stage_reserve, an unknown step code, ...) changes nothing:
 *     not the visible state, and not the ELBO parts of the call before it.
 */
#ifndef VIREO_HIP_H
#define VIREO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vrx_problem vrx_problem; /* AD/DP resident in HBM, both orientations   */
typedef struct vrx_model vrx_model;     /* variational state + priors + scratch in HBM */
typedef struct vrx_comm vrx_comm;       /* RCCL communicator (restart shard)           */

#define VRX_OK 0
#define VRX_ERR_ARG (-1)
#define VRX_ERR_HIP (-2)
#define VRX_ERR_NOMEM (-3)
#define VRX_ERR_UNSUPPORTED (-4)
#define VRX_ERR_COMM (-5)

const char* vrx_last_error(void);
int vrx_device_count(int* n);
/* name / CU count / HBM bytes of a device (for logs and bench.py) */
int vrx_device_info(int device, char* name, int name_len, int* n_cu, int64_t* hbm_bytes);

/* PCI bus id ("0000:c1:00.0") of a device: the physical GPU behind a rank of the restart shard
 * (the reference's pool workers are anonymous, vireo_wrap.py:74-83; a multi-GPU record must say
 * which GPUs it ran on). */
int vrx_device_pci_bus_id(int device, char* out, int out_len /* >= 16 */);

/* ---- the sparse count matrices -------------------------------------------------------
 * AD and DP (n_var x n_cell), given once, as ONE CSC pattern (the union of both patterns,
 * row indices strictly increasing inside a column) carrying an (ad, dp) pair per entry.
 * Replaces: the scipy.sparse operands of Vireo.fit (vireoSNP/utils/vireo_model.py:278)
 * and BinomMixtureVB.fit (vireoSNP/utils/bmm_model.py:204); "BD = DP - AD"
 * (vireo_model.py:168,190,228; bmm_model.py:122,136) is never materialised.
 * Builds the variant-major (CSR) copy and the segment tables on the way in. */
int vrx_problem_create(int device, int64_t n_var, int64_t n_cell, int64_t nnz,
                       const int64_t* csc_colptr /* n_cell+1 */,
                       const int32_t* csc_rowidx /* nnz */,
                       const int32_t* ad /* nnz */, const int32_t* dp /* nnz */,
                       vrx_problem** out);
/* The same with build options.  VRX_PROBLEM_BALANCED: *balanced slabs* -- for problems that run the
 * LDS-resident passes with AD/BD words and no split rows, the builder chooses PER ROW TILE which
 * contracted rows share a slab so that every row of the tile carries about the same number of words in
 * every slab (the passes execute a round of 16 rows at the pace of its longest row: 1.62 -> ~1.2 executed
 * slots per word at c3, passes 10-17 % shorter).  Costs a one-off ~0.5 s at 1e8 entries, so it pays from a
 * few thousand iterations on the same problem (vireo_wrap's restarts, vireo_wrap.py:64-94, all run on one);
 * results differ from the unbalanced build's in summation order only (<= 1e-13 relative per update).
 * The reference has no counterpart (SciPy's CSC / CSR are what they are). */
#define VRX_PROBLEM_BALANCED 1
int vrx_problem_create2(int device, int64_t n_var, int64_t n_cell, int64_t nnz,
                        const int64_t* csc_colptr, const int32_t* csc_rowidx, const int32_t* ad,
                        const int32_t* dp, int32_t flags, vrx_problem** out);
/* info4 = { variant stream balanced (0 | 1), cell stream balanced, seconds the balancing added to the build,
 * built on the device (0 | 1) } */
int vrx_problem_build_info(vrx_problem* p, double* info4);
/* fmt2 = { entry format of the variant orientation, of the cell orientation }: 0 = 4 B, 1 = 8 B, 2 = 12 B per
 * entry; the narrowest that holds the counts and the index, or the wider one VIREO_ENTRY_FMT asked for */
int vrx_problem_entry_format(vrx_problem* p, int32_t* fmt2);
void vrx_problem_destroy(vrx_problem* p);

/* sum over entries with dp>0 of float32(min(log C(dp,ad), 700)), accumulated in float64.
 * Replaces: np.sum(get_binom_coeff(AD, DP))  (vireoSNP/utils/vireo_base.py:7-22; called at
 * vireo_model.py:313 and bmm_model.py:239).  Computed once per problem and cached. */
int vrx_problem_binom_const(vrx_problem* p, double* sum_out);

/* Checksums (64-bit FNV-1a) of the device-resident problem, per orientation (variant-major
 * first): packed entries, tiled stream words, stream boundaries, wave starts, row map followed by
 * the balanced slabs' permutation (nothing when the stream is not balanced), number of gather
 * segments.  Two builds of one input are identical iff the first five agree; the tests hold the
 * device builder (vrx_build.h) to the host builder with it. */
int vrx_problem_digest(vrx_problem* p, uint64_t* out12);
/* per-cell count of variants with dp>0 (vireoSNP/vireo.py:191, "n_vars") */
int vrx_problem_n_vars(vrx_problem* p, int32_t* out /* n_cell */);

/* ---- model ------------------------------------------------------------------------- */
#define VRX_KIND_VIREO 0 /* class Vireo            vireoSNP/utils/vireo_model.py:11 */
#define VRX_KIND_BMM 1   /* class BinomMixtureVB   vireoSNP/utils/bmm_model.py:9    */

typedef struct {
    int32_t kind;         /* VRX_KIND_*                                                  */
    int32_t n_donor;      /* K                                                           */
    int32_t n_gt;         /* T (Vireo only; vireo_model.py:61)                           */
    int32_t learn_gt;     /* Vireo.learn_GT      (vireo_model.py:65)                     */
    int32_t learn_theta;  /* Vireo.learn_theta   (vireo_model.py:67)                     */
    int32_t ase_mode;     /* Vireo.ASE_mode      (vireo_model.py:66): theta per variant  */
    int32_t fix_beta_sum; /* fix_beta_sum        (vireo_model.py:68, bmm_model.py:52)    */
    int32_t n_batch;      /* restarts held by ONE model (0 or 1: a single model; <= 16).  The
                             random restarts of vireo_wrap (vireo_wrap.py:64-87) fitted side by
                             side: state arrays gain a restart axis -- ID_prob [n_cell][R][K],
                             GT_prob [n_var][R][K][T], beta [R][rows][cols], logLik_ID
                             [n_cell][R][K] -- and fit / run_iters / step(ELBO) / get_elbo_parts
                             return one trace / value per restart                           */
} vrx_model_cfg;

int vrx_model_create(vrx_problem* p, const vrx_model_cfg* cfg, vrx_model** out);
void vrx_model_destroy(vrx_model* m);

/* Upload the variational state (attributes ID_prob, GT_prob, beta_mu, beta_sum of the
 * reference objects: vireo_model.py:84-104, bmm_model.py:69-83).  A NULL pointer leaves
 * that array as it is on the device.  GT_prob is ignored for VRX_KIND_BMM. */
int vrx_model_set_state(vrx_model* m, const double* ID_prob, const double* GT_prob,
                        const double* beta_mu, const double* beta_sum);
/* Initial state straight from the random draws (Vireo.set_initial, vireo_model.py:98-104:
 * ID_prob = normalize(rand(M, K)), GT_prob = normalize(rand(N, K, T))): uploads the RAW draws
 * and normalises them on the device over the last axis, bit-identically to NumPy's
 * X / X.sum(-1) (pairwise summation order restated in vrx_normalize_rows).  NULL arguments are
 * left untouched.  <= 128 columns. */
int vrx_model_set_state_raw(vrx_model* m, const double* ID_raw, const double* GT_raw,
                            const double* beta_mu, const double* beta_sum);
/* Staged uploads for back-to-back restarts (vireo_wrap.py:64-87 constructs and fits n_init models
 * one after the other): the raw draws of restart i + 1 travel to the device while restart i fits.
 * stage_reserve: once, from the thread that owns the model (single Vireo models): two staging
 * buffers, a copy stream.  stage_raw: buffer buf (0 | 1) <- the raw draws; MAY BE CALLED FROM A SECOND
 * HOST THREAD while vrx_model_fit runs on the same model (it touches only the staging buffer and the
 * copy stream; it returns when the host arrays may be reused).  set_state_staged: the model's
 * state <- normalised buffer buf (+ beta_mu / beta_sum, NULL = untouched): the same bits as
 * vrx_model_set_state_raw from the same draws. */
int vrx_model_stage_reserve(vrx_model* m);
int vrx_model_stage_raw(vrx_model* m, int32_t buf, const double* ID_raw, const double* GT_raw);
int vrx_model_set_state_staged(vrx_model* m, int32_t buf, const double* beta_mu, const double* beta_sum);
/* restore == 0: save (ID_prob, GT_prob, beta_mu, beta_sum) in a device-side slot;
 * restore != 0: bring them back.  The best restart so far (vireo_wrap.py:90-91) stays in HBM. */
int vrx_model_snapshot(vrx_model* m, int32_t restore);
int vrx_model_get_state(vrx_model* m, double* ID_prob, double* GT_prob, double* beta_mu,
                        double* beta_sum);
/* Restart batches (vrx_model_cfg.n_batch = R > 1).  vireo_wrap.py:64-87 builds n_init models
 * and fits them one after the other; here R of them share every sparse pass.
 * set_restart: slot r <- one restart's state, in the SINGLE-model layouts of
 * vrx_model_set_state (raw == 0) or vrx_model_set_state_raw (raw != 0: normalised on the
 * device).  copy_restart: the single model dst <- slot r of src, device to device (the
 * winner, vireo_wrap.py:90-91).  Prior tables (vrx_model_set_prior) are shared by the batch. */
int vrx_model_set_restart(vrx_model* m, int32_t r, const double* ID, const double* GT,
                          const double* beta_mu, const double* beta_sum, int32_t raw);
int vrx_model_copy_restart(vrx_model* dst, vrx_model* src, int32_t r);

/* Priors (Vireo.set_prior vireo_model.py:107-137; BinomMixtureVB.set_prior
 * bmm_model.py:87-105).  ID_prior: id_rows = 0 -> uniform 1/K (pointer ignored), 1 -> one
 * row broadcast to every cell, n_cell -> full.  GT_prior: gt_rows = 0 -> uniform 1/T,
 * 1 -> one (K,T) slab broadcast over variants, n_var -> full.  Priors are given as
 * probabilities (not logs); rows are re-normalised for the KL terms exactly like
 * scipy.stats.entropy does (vireo_model.py:237-238).  theta priors have the shape of
 * beta_mu (prior_rows = 1 or the state's row count). */
int vrx_model_set_prior(vrx_model* m, const double* ID_prior, int64_t id_rows,
                        const double* GT_prior, int64_t gt_rows,
                        const double* theta_s1_prior, const double* theta_s2_prior,
                        int64_t theta_prior_rows);

/* The coordinate-ascent loop.
 * Replaces Vireo._fit_VB (vireo_model.py:251-276) / BinomMixtureVB._fit_BV
 * (bmm_model.py:178-201): same update order, same convergence test, same "it" on exit.
 *   elbo_trace[0 .. *it_out] receives EVERY computed ELBO (without the binomial
 *   constant), i.e. one more than the reference keeps: the reference returns
 *   ELBO[:it] -- the host mirrors that truncation.
 *   warn_flags: bit0 = "lower bound decreases" seen, bit1 = "did not converge".
 * Continues from the state currently on the device (warm restart, vireo_wrap.py:94).
 * A batch model (n_batch = R) runs until its last restart has stopped; a restart that has
 * stopped is frozen (its kernels return at once).  Outputs are then per restart:
 * elbo_trace [R][max_iter], it_out [R], warn_flags [R]. */
int vrx_model_fit(vrx_model* m, int32_t max_iter, int32_t min_iter, double epsilon_conv,
                  int32_t delay_fit_theta, double* elbo_trace /* [R][max_iter] */,
                  int32_t* it_out /* [R] */, int32_t* warn_flags /* [R] */);

/* Single coordinate updates, for the public step methods:
 *   VRX_STEP_THETA  Vireo.update_theta_size (vireo_model.py:165) / bmm_model.py:133
 *   VRX_STEP_GT     Vireo.update_GT_prob    (vireo_model.py:204)
 *   VRX_STEP_ID     Vireo.update_ID_prob    (vireo_model.py:187) -> logLik_ID kept on device
 *                   BMM: get_E_logLik + update_ID_prob (bmm_model.py:118,147)
 *   VRX_STEP_LOGLIK recompute logLik_ID only (get_ELBO(None, AD, DP), vireo_model.py:227)
 *   VRX_STEP_ELBO   get_ELBO with the logLik_ID on the device (vireo_model.py:236-248) */
#define VRX_STEP_THETA 1
#define VRX_STEP_GT 2
#define VRX_STEP_ID 3
#define VRX_STEP_LOGLIK 4
#define VRX_STEP_ELBO 5
#define VRX_STEP_SOFTMAX 6 /* ID_prob <- softmax(logLik_ID on device + log ID_prior): the tail of
                              update_ID_prob alone (bmm_model.py:153-154 with logLik_ID given) */
int vrx_model_step(vrx_model* m, int32_t which, double* elbo_out /* VRX_STEP_ELBO only */);
/* logLik_ID as the call that defined it last left it (see Conventions): a step, the last
 * iteration of a fit or of vrx_model_run_iters, or vrx_model_set_loglik.  Single models. */
int vrx_model_get_loglik(vrx_model* m, double* logLik_ID /* n_cell x n_donor */);
int vrx_model_set_loglik(vrx_model* m, const double* logLik_ID);
/* the four ELBO terms of the last VRX_STEP_ELBO / fit iteration:
 * LB_p, KL_ID, KL_GT, KL_theta (vireo_model.py:236-245); [R][4] for a batch.  Defined only
 * straight after the call that computed that ELBO (see Conventions). */
int vrx_model_get_elbo_parts(vrx_model* m, double* parts4);

/* Doublet scoring with a fitted model, the device form of predict_doublet
 * (vireoSNP/utils/vireo_doublet.py:11-82): the genotype table of all donor pairs
 * (add_doublet_GT, :105-136) is formed on the fly inside the kernel that builds the cell
 * pass's W tables; logLik / prob_out are (n_cell x C), C = K + K(K-1)/2 (singlets first,
 * pairs in itertools.combinations order).  psi*: digammas of the T + T(T-1)/2 class thetas
 * of add_doublet_theta (:85-102), (psi_rows x G).  n_donor >= 2; every n_gt a model can have
 * (1 .. 8, so G <= 36): the classes are formed one at a time, never as a table. */
int vrx_problem_doublet(vrx_problem* p, int64_t n_donor, int64_t n_gt,
                        const double* GT_prob /* n_var x n_donor x n_gt */,
                        const double* psi1, const double* psi2, const double* psis,
                        int64_t psi_rows /* 1 or n_var */,
                        const double* ID_prior, int64_t id_rows,
                        double* logLik, double* prob_out /* may be NULL */);

/* Expected reads per variant and donor: AD @ ID_prob and DP @ ID_prob, (n_var x n_col) each
 * -- one variant pass.  Replaces the two products the command line makes for the donor VCF
 * (vireoSNP/vireo.py:240-241, "cell_dat['AD'] * res_vireo['ID_prob']"). */
int vrx_problem_donor_reads(vrx_problem* p, int64_t n_col, const double* ID_prob,
                            double* AD_reads, double* DP_reads);

/* One-shot cell log-likelihood against caller-supplied genotype/theta tables:
 *   logLik[m,c] = sum_n sum_g GT[n,c,g] * (AD[n,m] psi1[g] + BD[n,m] psi2[g] - DP[n,m] psis[g])
 * with psi*(n_rows_psi x G): the 3*G transposed products of predict_doublet
 * (vireoSNP/utils/vireo_doublet.py:53-62); any n_col >= 1 and n_class <= 8 (the class limit of the
 * dense kernels: an explicit doublet table fits for n_GT <= 3 only, G = T + T(T-1)/2 = 6 classes --
 * predict_doublet uses vrx_problem_doublet, which has no such limit).
 * If prob_out is non-NULL it receives softmax_c(logLik + log ID_prior)
 * (vireo_doublet.py:67-68; ID_prior rows as in vrx_model_set_prior). */
int vrx_problem_cell_loglik(vrx_problem* p, int64_t n_col, int64_t n_class,
                            const double* GT /* n_var x n_col x n_class */,
                            const double* psi1, const double* psi2, const double* psis,
                            int64_t psi_rows /* 1 or n_var */,
                            const double* ID_prior, int64_t id_rows,
                            double* logLik /* n_cell x n_col */,
                            double* prob_out /* n_cell x n_col, may be NULL */);

/* ---- ambient RNA (vrx_ambient.h) ---------------------------------------------------------
 * vrx_problem_elbo_gain: gain[n_var] of variant_ELBO_gain(ID_prob, AD, DP, pseudocount)
 * (vireoSNP/utils/variant_select.py:66-106): one variant pass for AD@ID, DP@ID and the row sums
 * (BD@ID = DP@ID - AD@ID), then the digamma / logsumexp per variant on the device. */
int vrx_problem_elbo_gain(vrx_problem* p, int64_t n_col, const double* ID_prob /* n_cell x n_col */,
                          double pseudocount, double* gain /* n_var */);
/* The per-cell EM of predit_ambient (vireoSNP/utils/vireo_doublet.py:213-273, _fit_EM_ambient :139-210),
 * every cell in one launch: the cells' entries of the selected variants with dp > 0 are compacted from the
 * problem's cell orientation (count, scan, scatter), then one wave per cell runs the EM from psi_init
 * with the reference's stop rule (min_iter, max_iter, epsilon), its returned log-likelihood
 * logLik[it - 1], the Cramer-Rao variance and the likelihood ratio against the one-hot psi at the
 * first maximum.  theta: n_var x n_donor (the caller's np.tensordot(GT_prob, beta_mu[0])), selected: one
 * byte per variant.  n_iter: the reference's loop index at exit.  A cell without selected counts gets
 * NaN psi / var / llr and n_iter = max_iter - 1, as in the reference.  ms3 (may be NULL): milliseconds of
 * the compaction, the EM kernel and the download. */
int vrx_problem_ambient(vrx_problem* p, int64_t n_donor, const double* theta, const uint8_t* selected,
                        const double* psi_init /* n_cell x n_donor */, int32_t min_iter, int32_t max_iter,
                        double epsilon, double* psi /* n_cell x n_donor */, double* var /* n_cell x n_donor */,
                        double* llr /* n_cell */, int32_t* n_iter /* n_cell */, double* ms3);
/* What vrx_problem_ambient launches at n_donor under the environment as it is (VIREO_AMBIENT_LDS): cap, the
 * most selected entries of a cell whose theta rows stay in LDS (a longer cell reads them from global memory),
 * and the LDS bytes of one cell's wave.  Reads nothing of the device. */
int vrx_ambient_info(int64_t n_donor, int32_t* cap, int64_t* lds_bytes);

/* ---- bulk donor abundance (vrx_bulk.h) ---------------------------------------------------
 * A bulk sample's per-variant counts and the donors' genotype probabilities, resident on the
 * device: the operands of VireoBulk.fit (vireoSNP/utils/vireo_bulk.py:44-108) and LikRatio_test
 * (:120-167).  GT_prob is n_var x n_donor x n_gt, AD / DP are n_var doubles ("BD = DP - AD",
 * :72 and :151, is formed on the way in).  n_donor >= 1, n_gt >= 2. */
typedef struct vrx_bulk vrx_bulk;
int vrx_bulk_create(int device, int64_t n_var, int64_t n_donor, int64_t n_gt, const double* GT_prob,
                    const double* AD, const double* DP, vrx_bulk** out);
void vrx_bulk_destroy(vrx_bulk* b);
/* another sample on the same genotypes (GT_prob stays where it is) */
int vrx_bulk_set_counts(vrx_bulk* b, const double* AD, const double* DP);
/* The EM loop of VireoBulk.fit (vireo_bulk.py:75-105) from psi_io / theta_io, which receive the
 * fitted values.  One pass over GT_prob per iteration plus one: pass p yields logLik[p - 1] and
 * the sums of update p; the stop rule (:97-105, same order of comparisons) runs on the device.
 * logLik_trace[0 .. last_it] are the reference's logLik[0 .. it]; last_it is its loop index at
 * exit.  ms_out (may be NULL): device milliseconds from the first pass to the last. */
int vrx_bulk_fit(vrx_bulk* b, double* psi_io /* n_donor */, double* theta_io /* n_gt */, int32_t max_iter,
                 int32_t min_iter, double epsilon, int32_t learn_theta, int32_t delay_fit_theta,
                 double* logLik_trace /* max_iter */, int32_t* last_it, double* ms_out);
/* sum_n AD log(t) + BD log(1 - t), t = GT_prob . theta . psi (vireo_bulk.py:94-96, :152-158), for
 * n_psi vectors at once (eight per pass over GT_prob). */
int vrx_bulk_loglik(vrx_bulk* b, int64_t n_psi, const double* psi /* n_psi x n_donor */,
                    const double* theta /* n_gt */, double* out /* n_psi */);
/* A cohort: n_sample bulk samples genotyped against the same donors, the loop over samples that
 * users of VireoBulk write around :44-108 (one fit per sample on the same GT_prob).  AD / DP are
 * n_sample x n_var doubles ("BD = DP - AD", :72, formed on the way in).  Replaces any earlier
 * cohort; the handle's single-sample counts, vrx_bulk_fit and vrx_bulk_loglik are untouched by it.
 * Fails with the LDS message where n_donor x n_gt is too large for a chunk's accumulators. */
int vrx_bulk_set_cohort(vrx_bulk* b, int64_t n_sample, const double* AD /* n_sample x n_var */,
                        const double* DP /* n_sample x n_var */);
/* samples that share one read of a GT_prob tile (a compile-time constant) */
int32_t vrx_bulk_cohort_chunk(void);
/* The EM loop of VireoBulk.fit (vireo_bulk.py:75-105) for every sample of the cohort at once, each
 * from its own row of psi_io / theta_io, which receive the fitted values.  The stop rule (:97-105)
 * runs per sample on the device; a sample that has stopped is frozen while the others go on.
 * logLik_trace row s holds that sample's logLik[0 .. last_it[s]] and zeros behind it.  A sample's
 * results do not depend on the other samples of the cohort nor on its position among them. */
int vrx_bulk_fit_cohort(vrx_bulk* b, double* psi_io /* n_sample x n_donor */, double* theta_io /* n_sample x n_gt */,
                        int32_t max_iter, int32_t min_iter, double epsilon, int32_t learn_theta,
                        int32_t delay_fit_theta, double* logLik_trace /* n_sample x max_iter */,
                        int32_t* last_it /* n_sample */, double* ms_out);
/* The log-likelihood of vireo_bulk.py:94-96 / :152-158 for n_psi vectors per sample, each sample under
 * its own theta and counts (LikRatio_test for a whole cohort in one pass per eight vectors). */
int vrx_bulk_loglik_cohort(vrx_bulk* b, int64_t n_psi, const double* psi /* n_sample x n_psi x n_donor */,
                           const double* theta /* n_sample x n_gt */, double* out /* n_sample x n_psi */);
/* Variants per tile and workgroups of the four passes, as the handle launches them: T, n_wg (fit), T_ll,
 * n_wg_ll (log-likelihood), T_co, n_wg_co, T_co_ll, n_wg_co_ll (the cohort's).  Reads the handle only. */
int vrx_bulk_info(const vrx_bulk* b, int32_t out[8]);

/* ---- donor matching (vrx_match.h) -----------------------------------------------------------
 * The genotype distance between every donor of X and every donor of Z,
 *   D[i][j] = mean over (n, t) of |X[n][i][t] - Z[n][j][t]|,
 * in one streaming pass over both tensors: the matrix that optimal_match fills pair by pair with
 * np.mean(np.abs(...)) (vireoSNP/utils/vireo_base.py:197-201; called by match_VCF_samples,
 * vcf_utils.py:404-405) and, with Z = X, the one of donor_select (vireo_base.py:230-234).
 * The operands stay on the host: the call walks them in slabs of block_vars variants (default: the
 * most that keep each operand's slab at or below 256 MiB), uploads a slab of each, adds the slab's
 * partial sums and reduces chunks and slabs in order -- no atomics, so two calls with the same
 * block_vars on the same device are bitwise identical.  A NaN reaches exactly the cells of the donor
 * that carries it.  n_var, k1, k2, n_gt >= 1; VRX_ERR_UNSUPPORTED when one variant of a 4 x 4 donor
 * tile does not fit the kernel's LDS (n_gt in the hundreds). */
int vrx_geno_dist(int device, int64_t n_var, int64_t k1, int64_t k2, int64_t n_gt,
                  const double* X /* host, n_var x k1 x n_gt */,
                  const double* Z /* host, n_var x k2 x n_gt; NULL: Z = X, k2 = k1 */,
                  int64_t block_vars /* variants per upload slab; 0: default */,
                  double* D /* host, k1 x k2 */, double* ms_out /* kernel ms, may be NULL */);

/* ---- barcode selection (vrx_barcode.h) -----------------------------------------------------
 * The greedy rounds of variant_select (vireoSNP/utils/variant_select.py:22-62).  A handle keeps the
 * categorical genotypes (values 0..9, n_donor <= 128) and the optional var_count on the device; the
 * host keeps only a class rank per donor (donors with equal barcodes so far share a class, classes
 * in the string order of their barcodes).
 * vrx_barcode_create: GT is DONOR-major, n_donor x n_var bytes; var_count n_var doubles or NULL.
 * vrx_barcode_round replaces the loop over all variants with barcode_entropy (:42-44, :5-19) and the
 * tie set, median filter and count of :45-52: every variant's entropy is the reference's double,
 * bit for bit -- the terms in np.unique's order, both sums by np.sum's rule, and entr() read from
 * `table`, (2 H + 1) x (n_donor + 1) doubles the host filled with scipy.special.entr:
 * table[j + H][c] = entr((c / n_donor) / s_j), s_j the double with the bit pattern of 1.0 plus j.
 * `order`: the donors sorted by class; `bnd`: n_class + 1 boundaries of the classes in it; `log2`:
 * np.log(2).  Out: the maximal entropy and counts3 = variants tied at it (by value), those of them
 * with var_count >= np.median of the tied counts (all of them without var_count), variants whose
 * normalising sum lies more than H ulp from 1.  If the last is not 0 the call fails with
 * VRX_ERR_UNSUPPORTED: no entropy is ever evaluated approximately.  ms2 (may be NULL): milliseconds of
 * the entropy kernel and of the kernels after it.
 * vrx_barcode_pick: `idx[np.random.randint(len(idx))]` (:53) once the host has drawn r: the r-th
 * survivor in ascending variant index, and its entropy (:57).
 * vrx_barcode_entropies: the last round's per-variant entropies (n_var doubles); for the tests. */
typedef struct vrx_barcode vrx_barcode;
int vrx_barcode_create(int device, int64_t n_var, int64_t n_donor, int64_t n_cat /* 1 + largest value */,
                       const uint8_t* GT, const double* var_count, vrx_barcode** out);
void vrx_barcode_destroy(vrx_barcode* b);
int vrx_barcode_round(vrx_barcode* b, const int32_t* order /* n_donor */, const int32_t* bnd /* n_class + 1 */,
                      int32_t n_class, const double* table, int32_t half_width /* H */, double log2,
                      double* max_out, int64_t* counts3, double* ms2);
int vrx_barcode_pick(vrx_barcode* b, int64_t r, int64_t* index_out, double* entropy_out);
int vrx_barcode_entropies(vrx_barcode* b, double* out /* n_var */);

/* ---- per-variant clone mixtures (vrx_varmix.h) ----------------------------------------------
 * BinomMixtureVB._fit_BV (vireoSNP/utils/bmm_model.py:178-201) on every variant's own 1 x n_cell row,
 * with default priors (set_prior, :87-105), fix_beta_sum = False and a start computed from the counts,
 * against the same bound with n_donor = 1: the "M1 multiple donors vs M0 single donor" of
 * variant_ELBO_gain (variant_select.py:66-106) with the assignment learned per variant.
 * vrx_varmix_create: a CSR of the covered entries only (dp > 0, 0 <= ad <= dp, in increasing cell
 * index); no column indices -- update_theta_size (:133-144), get_E_logLik (:118-130), update_ID_prob
 * (:147-154) and get_ELBO (:157-175) never ask which cell an entry is, and a cell without reads adds
 * exactly nothing to any of them.  n_var = 0 and nnz = 0 are legal; an invalid entry or a rowptr that
 * is not monotone from 0 to nnz is VRX_ERR_ARG.
 * vrx_varmix_wave_rows: the longest row one wavefront fits; longer rows take a workgroup (a
 * compile-time constant).
 * vrx_varmix_fit: one launch fits every row with n_clone components from
 *   ID_init_ik = w_k / sum_k w_k,  w_k = max(0, 1 - |a_i / d_i - k / (K - 1)| (K - 1)) + 1/64
 * (what ID_prob_init would be, :80-81) and evaluates the stop rule of :190-199 per row on the device.
 * Per row: n_iter = `it` at exit; elbo_k = ELBO[it - 1], the reference's ELBO_iters[-1] (:201);
 * elbo_one = the value _fit_BV records at every iteration with n_donor = 1 (closed form); beta_mu,
 * beta_sum of iteration `it`; size = sum of ID_prob of iteration `it` over the covered cells; warn
 * bit 0: the bound decreased by more than 1e-6 (:191), bit 1: not converged (:195); trace (may be
 * NULL) = ELBO[0 .. it], zeros after it.  An empty row returns elbo 0, beta_mu 0.5, beta_sum 2,
 * size 0.  Results are bitwise a function of the row's entries and the parameters.  n_clone outside
 * 2 ... 8 or max_iter < 2: VRX_ERR_UNSUPPORTED.  ms (may be NULL): milliseconds of the kernel. */
typedef struct vrx_varmix vrx_varmix;
int vrx_varmix_create(int device, int64_t n_var, int64_t nnz, const int64_t* rowptr /* n_var + 1 */,
                      const int32_t* ad, const int32_t* dp, vrx_varmix** out);
void vrx_varmix_destroy(vrx_varmix* h);
int32_t vrx_varmix_wave_rows(void);
int vrx_varmix_fit(vrx_varmix* h, int32_t n_clone, int32_t max_iter, int32_t min_iter, double epsilon_conv,
                   double* elbo_k, double* elbo_one,                /* n_var each */
                   double* beta_mu, double* beta_sum, double* size, /* n_var x n_clone, any may be NULL */
                   int32_t* n_iter, int32_t* warn,                  /* n_var */
                   double* trace /* n_var x max_iter or NULL */, double* ms /* kernel ms or NULL */);

/* ---- SNP-to-gene matching and gene-level counts (vrx_genematch.h) ----------------------------
 * snp_gene_match (vireoSNP/utils/vcf_utils.py:423-491): the Python loop over SNPs, each forming its
 * distance to every gene of its chromosome once per gap (:466-482), as two launches over all SNPs.
 * Integers only; every result equals the reference's.
 * vrx_genematch_create: the genes grouped by chromosome code (gene_df[gene_df['chrom'] == _chrom],
 * :461, for every chromosome at once): chrom_ptr[c] .. chrom_ptr[c + 1] are the genes of code c in
 * gene_df row order, row[] their gene_df rows; start, stop and row in [0, 2^31 - 1].  n_gene = 0 and a
 * code without genes are legal.
 * vrx_genematch_tile / _block: genes of one LDS tile, SNPs of one workgroup (compile-time constants).
 * vrx_genematch_match: the SNPs sorted by code (code[] non-decreasing, pos[] in [0, 2^31 - 1]);
 * perm[j] = the index the results of the j-th sorted SNP are written at (a permutation).  gap_m1[k] =
 * gaps[k] - 1 clamped to the int32 range ("dist < gap", :475, as dist <= gap - 1); single[k] != 0 where
 * gaps[k] > 0 or multi_gene is False (:477).  flag[i] (:467, :485) and count[i] = len(idx_chrom)
 * (:475-481) per SNP in the caller's order.  The handle keeps what the second call needs.
 * vrx_genematch_lists: rows[] = the gene_df rows of idx_chrom (:488), SNP after SNP in the caller's order,
 * `total` = the sum of the counts of the match before it (anything else: VRX_ERR_ARG).
 * ms (may be NULL): milliseconds of the kernels of the call.
 *
 * vrx_genecount_*: what follows the matching in gene-level ASE, G @ AD and G @ DP with G[g, v] = the
 * number of times gene g is listed for variant v (the SciPy products of a 0/1 gene x SNP matrix).
 * vrx_genecount_create: the merged CSC of vrx_merge_counts (variants x cells) and the map as a CSR over
 * variants (gptr[v] .. gptr[v + 1] index gid[], gene numbers in [0, n_gene)).  Expands every entry to
 * its genes, sorts by (cell, gene) and adds equal keys in 64 bits.  n_out: distinct (cell, gene) pairs.
 * vrx_genecount_read: key = cell * n_gene + gene, ascending (column-major), and the two sums. */
typedef struct vrx_genematch vrx_genematch;
int vrx_genematch_create(int device, int64_t n_chrom, int64_t n_gene, const int64_t* chrom_ptr /* n_chrom + 1 */,
                         const int32_t* start, const int32_t* stop, const int32_t* row, vrx_genematch** out);
void vrx_genematch_destroy(vrx_genematch* h);
int32_t vrx_genematch_tile(void);
int32_t vrx_genematch_block(void);
int vrx_genematch_match(vrx_genematch* h, int64_t n_snp, const int32_t* code, const int32_t* pos,
                        const int32_t* perm, int32_t n_gap, const int32_t* gap_m1, const uint8_t* single,
                        int32_t* flag /* n_snp */, int64_t* count /* n_snp */, double* ms);
int vrx_genematch_lists(vrx_genematch* h, int64_t total, int32_t* rows /* total */, double* ms);
typedef struct vrx_genecount vrx_genecount;
int vrx_genecount_create(int device, int64_t n_var, int64_t n_cell, int64_t n_gene,
                         const int64_t* colptr /* n_cell + 1 */, const int32_t* rowidx, const int32_t* ad,
                         const int32_t* dp, const int64_t* gptr /* n_var + 1 */, const int32_t* gid,
                         vrx_genecount** out, int64_t* n_out, double* ms);
int vrx_genecount_read(vrx_genecount* h, int64_t* key, int64_t* ad, int64_t* dp /* n_out each */);
void vrx_genecount_destroy(vrx_genecount* h);

/* ---- pooling cell columns of several samples (vrx_pool.h) ---------------------------------------
 * The matrix-level counterpart of simulate/synth_pool.py: its BAM step only rewrites each read's cell
 * tag to the pooled barcode (:126-141) and pile-up is additive over reads, so on a fixed variant list
 * the counts of a pooled cell are the sum of its source cells' columns.  Integers only.
 * vrx_pool_create: the merged CSC of vrx_merge_counts of every sample, concatenated along the columns
 * (n_src source cells; rows strictly increasing inside a column and below n_var, counts not negative:
 * anything else is VRX_ERR_ARG).  The handle keeps the sources on the device.
 * vrx_pool_run: pooled column j = source column src0[j], plus source column src1[j] unless that is -1,
 * on the union of their rows; a source may serve several pooled columns.  colptr_out: the n_pool + 1
 * offsets of the result.  bad = -1, or the smallest pooled column in which a sum reached 2^31 (the
 * result is then not to be used).  A pooled column is a function of its sources alone, bit for bit.
 * One launch covers the plan, so long columns + ceil(short columns / 4) must stay below 2^24 workgroups
 * (16.7 M long or 67 M short pooled columns); a larger plan is VRX_ERR_ARG and has to be run in parts.
 * ms (may be NULL): milliseconds of the kernels.
 * vrx_pool_read: the colptr_out[n_pool] entries of the run before it (rows increasing per column).
 * vrx_pool_wave_limit: the most source entries of a pooled column that one wavefront walks; above it a
 * workgroup does.  vrx_pool_scan_block: pooled columns per workgroup of the offset scan.  Both are
 * compile-time constants. */
typedef struct vrx_pool vrx_pool;
int vrx_pool_create(int device, int64_t n_var, int64_t n_src, const int64_t* colptr /* n_src + 1 */,
                    const int32_t* rowidx, const int32_t* ad, const int32_t* dp, vrx_pool** out);
void vrx_pool_destroy(vrx_pool* h);
int32_t vrx_pool_wave_limit(void);
int32_t vrx_pool_scan_block(void);
int vrx_pool_run(vrx_pool* h, int64_t n_pool, const int32_t* src0, const int32_t* src1 /* n_pool each */,
                 int64_t* colptr_out /* n_pool + 1 */, int64_t* bad, double* ms);
int vrx_pool_read(vrx_pool* h, int32_t* rowidx, int32_t* ad, int32_t* dp);

/* ---- donor VCF text (vrx_vcf.h) ---------------------------------------------------------------------
 * The decompressed text of a donor VCF -> the unnormalised genotype values of the lines whose variant
 * occurs in the cell data: what load_VCF (vcf_utils.py:80-159: the line loop, the id CHROM_POS_REF_ALT,
 * the biallelic filter, the tag counts), match_donor_VCF / match_SNPs (io_utils.py:10-39 over match(),
 * vireo_base.py:130-184) and the code conversion of parse_donor_GPb (vcf_utils.py:299-350) do one
 * Python string at a time.  The host inflates the file, reads the header and feeds whole lines in slabs;
 * the text stays on the device for one slab.
 * vrx_vcf_create: tag 0 GT / 1 PL / 2 GP; n_sample = the sample columns of the #CHROM line; the cell
 * variant ids as one byte buffer with n_ids + 1 offsets (n_ids = -1: no matching, every kept line is a
 * row); pl_table = the 4096 values 10 ** (-0.1 * d - 0.025) made by NumPy (PL only, else may be NULL).
 * The ids are hashed (64 bits) with the device function that hashes a line's id, sorted once, and equal
 * hashes compared on bytes.
 * vrx_vcf_begin: starts a pass over the file.  mode 0: ids as they are; 1: "chr" + cell id; 2: "chr" +
 * donor id (the retries of match_SNPs, in that order; the caller re-feeds the file when a pass matched
 * nothing); -1 with n_ids = -1.  *status = the status of the cell table.
 * vrx_vcf_slab: n_bytes (< 2^31 - 64) of whole lines; only the last line of the file may lack its line
 * end.  info[0] = kept lines (after the filter), info[1] = those whose FORMAT names the tag, info[2] =
 * matched lines, info[3] = status bits: 1 equal cell ids, 2 a cell variant claimed by a second line,
 * 4 equal hashes on different bytes, 8 a '#' line, 16 a line with fewer than 9 fields, 32 a non-ASCII
 * byte or a '\r' not followed by '\n'.  With a status the results of the pass are void (the caller uses
 * the host functions).  seconds (may be NULL): upload, kernels.
 * vrx_vcf_rows: the info[2] matched lines of the slab before it, in file order: gpb[row][sample][3],
 * slot = the cell variant (the line's ordinal without matching), line = its ordinal among the kept lines
 * of the file, flag 1 = outside the device's grammar (the caller parses the line; its gpb row is
 * undefined), span = the line's [start, end) bytes in the slab, line end included.  Accepted: '.', './.',
 * '.|.'; GT first and last character digits with sum <= 2; PL three unsigned integers <= 4095; GP three
 * digits[.digits] of at most 15 significant and 22 fractional digits (integer / exact power of ten, one
 * correctly rounded division).  A row is bitwise a function of its line.  seconds (may be NULL): kernels,
 * download.
 * vrx_vcf_chunk: bytes of a line a wavefront looks at per step (a compile-time constant). */
typedef struct vrx_vcf vrx_vcf;
int vrx_vcf_create(int device, int32_t tag, int32_t n_sample, int32_t biallelic_only, int64_t n_ids,
                   const char* id_bytes, const int64_t* id_off /* n_ids + 1 */, const double* pl_table /* 4096 */,
                   vrx_vcf** out);
void vrx_vcf_destroy(vrx_vcf* h);
int32_t vrx_vcf_chunk(void);
int vrx_vcf_begin(vrx_vcf* h, int32_t mode, int32_t* status);
int vrx_vcf_slab(vrx_vcf* h, const char* text, int64_t n_bytes, int64_t* info /* 4 */, double* seconds /* 2 */);
int vrx_vcf_rows(vrx_vcf* h, double* gpb, int64_t* slot, int64_t* line, int32_t* flag, int64_t* span,
                 double* seconds /* 2 */);

/* ---- cell VCF text (vrx_cellvcf.h) ------------------------------------------------------------------
 * The decompressed text of cellSNP's cells.vcf.gz -> the sparse AD / DP entries of its kept lines: what
 * load_VCF(sparse=True) (vcf_utils.py:80-159: the line loop, the biallelic filter, FixedINFO),
 * parse_sample_info (vcf_utils.py:12-57: one FORMAT for all lines, '.' and '.:.:.' are missing calls,
 * every other sample field is an entry of the cell it stands for) and read_sparse_GeneINFO
 * (vcf_utils.py:192-205: the text after the last comma of a subfield, '.' -> 0, float()) do one Python
 * string at a time.  The host inflates the file, reads the header and feeds whole lines in slabs, as for
 * vrx_vcf_*.
 * vrx_cellvcf_create: n_sample = the sample columns of the #CHROM line (>= 1).
 * vrx_cellvcf_format: the FORMAT bytes of the file's first kept line (1 ... 255 bytes; the host reads
 * that one line) and the positions of the two keys among its ':'-separated names.  Slabs fed before it
 * must hold no kept line: a kept line then counts as one with another FORMAT.
 * vrx_cellvcf_slab: n_bytes (< 2^31 - 64) of whole lines; only the last line of the file may lack its
 * line end.  A line's sample region is cut into segments of vrx_cellvcf_segment() bytes, a wavefront
 * each; results do not depend on the cut.  info[0] = kept lines, info[1] = entries, info[2] = kept lines
 * with a value outside the device's grammar, info[3] = status bits: 8 a '#' line, 16 a line with fewer
 * than 9 fields, 32 a non-ASCII byte or a '\r' not followed by '\n', 64 a kept line with other FORMAT
 * bytes, 128 a kept line whose sample-field count is not n_sample, 256 an entry with fewer subfields
 * than FORMAT has names.  With a status the results are void (the caller uses the host functions).
 * seconds (may be NULL): upload, kernels.
 * vrx_cellvcf_rows: the slab before it as CSR: indptr (info[0] + 1, within the slab), and per entry in
 * file order the cell and the values of the two keys ('.' or 1-9 decimal digits); per kept line flag 1 =
 * some value of the line is outside that grammar or a field is longer than the device walks (the caller
 * parses the line and overwrites its values: the entry count does not depend on the values), span = the
 * line's [start, end) bytes in the slab, line end included, off = the positions of its first nine tabs
 * (the ninth = the end when there is no sample field) and its end after rstrip().  seconds (may be
 * NULL): download.
 * vrx_cellvcf_segment: bytes of a sample region per wavefront (a compile-time constant). */
typedef struct vrx_cellvcf vrx_cellvcf;
int vrx_cellvcf_create(int device, int32_t n_sample, int32_t biallelic_only, vrx_cellvcf** out);
void vrx_cellvcf_destroy(vrx_cellvcf* h);
int32_t vrx_cellvcf_segment(void);
int vrx_cellvcf_format(vrx_cellvcf* h, const char* fmt, int32_t fmt_len, int32_t key0, int32_t key1);
int vrx_cellvcf_slab(vrx_cellvcf* h, const char* text, int64_t n_bytes, int64_t* info /* 4 */, double* seconds /* 2 */);
int vrx_cellvcf_rows(vrx_cellvcf* h, int64_t* indptr, int32_t* cell, int32_t* v0, int32_t* v1, int32_t* flag,
                     int64_t* span /* [rows][2] */, int32_t* off /* [rows][10] */, double* seconds /* 1 */);

/* ---- BGZF inflation (vrx_bgzf.h) ---------------------------------------------------------------------
 * A BGZF file (bgzip, cellSNP) is a chain of gzip members of at most 64 KiB of text each; a member's
 * header holds its compressed size, its footer the CRC32 and the length of its text.  The members are
 * independent: one wavefront inflates one member into LDS, holds it to the footer and writes it out.
 * vrx_bgzf_scan (host only): the members of the file image file[0, n_bytes).  Every member must begin
 * with the 18 bytes bgzip / htslib write (1f 8b 08 04, XLEN 6, subfield BC of length 2), and the chain of
 * their sizes must end exactly at n_bytes.  Returns VRX_OK and *status = 0, or *status = 1 a member with
 * another header (plain gzip, other flags, further subfields, trailing bytes), 2 a member cut short, 3 a
 * size the format does not allow.  *n_members = the whole members (in front of the fault); the first
 * `room` of them are stored (room = 0: counting only, the arrays may be NULL): payload_off / payload_len
 * = the deflate stream of each, isize = its footer's text length, out_off (room + 1 places) = the sum of
 * isize in front of it, the total at [*n_members].  A file without the empty end-of-file member is fine.
 * vrx_bgzf_create: max_text = the text bytes of one vrx_bgzf_inflate call (64 KiB ... 1 GiB; 0 = 256 MiB).
 * vrx_bgzf_inflate: a batch of n_members >= 1 members out of the n_comp < 2^31 compressed bytes at comp:
 * payload_off / payload_len as vrx_bgzf_scan gives them, relative to comp (each footer, the 8 bytes behind
 * the payload, lies inside comp); out_off (n_members + 1, non-decreasing from 0, steps of at most 64 KiB,
 * the last at most max_text) = where each member's text goes in text.  Both directions go through a
 * pinned buffer the handle owns.  status[i] = 0, or the bits of what the device could not vouch for in
 * member i (VRX_BGZF_ST_* in vrx_bgzf.h: 1 stream longer than the payload, 2 block type 3, 4 stored
 * LEN / NLEN, 8 code-length header, 16 over-subscribed, 32 incomplete, 64 no end-of-block code, 128 an
 * invalid symbol, 256 a distance before the first byte, 512 a write beyond ISIZE, 1024 fewer bytes than
 * ISIZE, 2048 payload bytes left over, 4096 CRC32, 8192 iteration cap, 16384 ISIZE is not the step of
 * out_off); the text of such a member is undefined, the other members are not affected.  seconds (may be
 * NULL): upload, kernels, download. */
typedef struct vrx_bgzf vrx_bgzf;
int vrx_bgzf_scan(const uint8_t* file, int64_t n_bytes, int64_t room, int64_t* n_members, int64_t* payload_off,
                  int32_t* payload_len, int32_t* isize, int64_t* out_off, int32_t* status);
int vrx_bgzf_create(int device, int64_t max_text, vrx_bgzf** out);
void vrx_bgzf_destroy(vrx_bgzf* h);
int vrx_bgzf_inflate(vrx_bgzf* h, const uint8_t* comp, int64_t n_comp, int64_t n_members, const int64_t* payload_off,
                     const int32_t* payload_len, const int64_t* out_off, uint8_t* text, int32_t* status,
                     double* seconds /* 3 */);

/* ---- timing (bench.py roofline leg) ---------------------------------------------------
 * When enabled, every launch of a pass kernel is bracketed by hipEvents on the model's
 * stream; totals are read back after a sync.  Kernel ids: */
#define VRX_KERN_VARIANT_PASS 0 /* variant-major sparse pass (AD,DP)*ID_prob          */
#define VRX_KERN_CELL_PASS 1    /* cell-major sparse pass (AD,DP)^T*W                 */
#define VRX_KERN_DENSE 2        /* all dense/epilogue kernels together                */
#define VRX_KERN_COUNT 3
/* which kernels this model's passes run: info[0]/[1] = 1 if the variant/cell pass is
 * LDS-resident (vrx_spmm_lds) else 0 (vrx_spmm, global gathers); info[2]/[3] = entry format
 * of the variant/cell orientation (0: 4 B, 1: 8 B, 2: 12 B per non-zero); info[4]/[5] =
 * L2 tiles of the variant/cell orientation; info[6]/[7] = partial arrays of the LDS-resident
 * variant/cell pass (the most pieces its work list cuts a tile into); info[8]/[9] = its stream
 * words (padding included) per 1000 non-zeros; info[10]/[11] = extra row pieces (long rows are
 * cut into interleaved pieces); info[12] = form of the LDS-resident cell stream (0: (ad, dp)
 * pairs, 1: single-valued AD / BD entries); info[13] = form of the variant stream (0: pairs,
 * 3: AD / BD entries as 2N single-accumulator virtual rows -- the cell pass's kernel); info[14] = restarts in the model (n_batch); info[15]
 * = longest / mean wave stream of the tiled streams x 1000 (variant: low 16 bits, cell: high 16).  The forms follow
 * the depth of the data: AD/BD words unless a count needs so many of them (> 1.56 words per
 * entry, estimated at vrx_problem_create) that one pair word per entry is cheaper. */
int vrx_model_info(vrx_model* m, int32_t* info16);
/* Which instances of vrx_spmm_lds the last LDS-resident pass of an orientation launched (orient 0: the
 * variant pass, 1: the cell pass), one record of VRX_LDS_LAUNCH_FIELDS values per column-block launch, in
 * launch order: the instance's template arguments MODE (the kernel's: 1 also for a variant pass over AD/BD
 * virtual rows), RW (rows per wave), PADK, SPLIT, FORM; then kb (columns of the block), ld (columns per
 * operand row), perm (1: the balanced gather list was passed), slab_rows and n_slab of the stream.  The
 * selection that returns the kernel returns these values with it.  *n_out = launches recorded (0: that
 * pass has not run on the LDS-resident path); at most `cap` records are written to out. */
#define VRX_LDS_LAUNCH_FIELDS 10
int vrx_model_lds_launches(vrx_model* m, int32_t orient, int32_t* out /* cap x VRX_LDS_LAUNCH_FIELDS */,
                           int32_t cap, int32_t* n_out);
/* What the dense kernels' last launches of each kind did (host bookkeeping, written where the launch is
 * enqueued; 0 / -1 until that kind has been launched).  out[VRX_DENSE_FIELDS], by index:
 *   N_CU          compute units the grid caps were formed for
 *   NB_THETA      blocks of the last theta kernel without the ELBO ride block (vrx_theta_partial; the
 *                 whole grid of vrx_theta_ase / vrx_bmm_theta)
 *   THETA_FINAL   how the last shared-theta update was finalised: VRX_DENSE_THETA_NONE (none yet, or a
 *                 kind that finalises inside its theta kernel), _FUSED (inside vrx_gt_update, VrxThetaFuse)
 *                 or _KERNEL (vrx_theta_final); THETA_PARTS = the stage-1 partials it summed
 *   NB_GT         blocks (= KL_GT partials) of the last vrx_gt_update
 *   NB_CELL, KP   blocks and lanes per cell of the last vrx_cell_softmax<KP>
 *   CELL_SOURCE   where the cell partials the next ELBO sums came from: VRX_DENSE_CELL_SOFTMAX or
 *                 VRX_DENSE_CELL_FUSED (the epilogue of the fused cell pass), -1 before either
 *   ELBO_CELL / _GT / _TH   the partial counts (per restart) the last vrx_elbo_final summed
 *   RIDE_CELL / _GT / _TH   the same of the last ELBO that rode as the extra block of the next theta launch
 *   ELBO_CARRIER  which of the two ran last: VRX_DENSE_ELBO_NONE, _KERNEL (vrx_elbo_final) or _RIDE        */
#define VRX_DENSE_N_CU 0
#define VRX_DENSE_NB_THETA 1
#define VRX_DENSE_THETA_FINAL 2
#define VRX_DENSE_THETA_PARTS 3
#define VRX_DENSE_NB_GT 4
#define VRX_DENSE_NB_CELL 5
#define VRX_DENSE_KP 6
#define VRX_DENSE_CELL_SOURCE 7
#define VRX_DENSE_ELBO_CELL 8
#define VRX_DENSE_ELBO_GT 9
#define VRX_DENSE_ELBO_TH 10
#define VRX_DENSE_RIDE_CELL 11
#define VRX_DENSE_RIDE_GT 12
#define VRX_DENSE_RIDE_TH 13
#define VRX_DENSE_ELBO_CARRIER 14
#define VRX_DENSE_FIELDS 15
#define VRX_DENSE_THETA_NONE 0
#define VRX_DENSE_THETA_FUSED 1
#define VRX_DENSE_THETA_KERNEL 2
#define VRX_DENSE_CELL_SOFTMAX 0
#define VRX_DENSE_CELL_FUSED 1
#define VRX_DENSE_ELBO_NONE 0
#define VRX_DENSE_ELBO_KERNEL 1
#define VRX_DENSE_ELBO_RIDE 2
int vrx_model_dense_launches(vrx_model* m, int32_t* out /* VRX_DENSE_FIELDS */);
int vrx_model_profile(vrx_model* m, int32_t enable);
int vrx_model_profile_read(vrx_model* m, double* ms_total /* VRX_KERN_COUNT */,
                           int64_t* launches /* VRX_KERN_COUNT */);
/* run `n_iter` full iterations with no convergence test and no host sync in between
 * (the timed region of bench.py); returns wall ms measured with hipEvents on the stream. */
int vrx_model_run_iters(vrx_model* m, int32_t n_iter, int32_t theta_from_iter,
                        double* elbo_trace /* n_iter */, double* ms_out);

/* ---- restart shard over RCCL ---------------------------------------------------------
 * vireo_wrap.py:74-91 farms n_init restarts to a multiprocessing.Pool and takes
 * argmax(ELBO_[-1]).  Here restarts are sharded one process per GPU and the per-restart
 * ELBOs are all-gathered over RCCL/xGMI. */
#define VRX_UNIQUE_ID_BYTES 128
int vrx_comm_unique_id(uint8_t* id /* VRX_UNIQUE_ID_BYTES */);
int vrx_comm_create(int device, int rank, int world, const uint8_t* id, vrx_comm** out);
void vrx_comm_destroy(vrx_comm* c);
/* all ranks contribute n_local doubles; out has world*n_local doubles, rank-major */
int vrx_comm_allgather_f64(vrx_comm* c, const double* local, int64_t n_local, double* out);
int vrx_comm_barrier(vrx_comm* c);
/* broadcast a host buffer of doubles from `root` (winner's state to rank 0 / everyone) */
int vrx_comm_bcast_f64(vrx_comm* c, double* buf, int64_t n, int root);

/* info4 = rank, world, device, librccl version code (ncclGetVersion; 0 = unknown) */
int vrx_comm_info(vrx_comm* c, int32_t* info4);
/* The winner's state to every rank, DEVICE TO DEVICE: vireo_wrap.py:90-94 continues with
 * `_models_all[_idx]`; here the owner of the best restart broadcasts ID_prob, GT_prob, beta_mu,
 * beta_sum straight from its model's HBM buffers into the same buffers of every other rank's model
 * (one RCCL group call, no host staging).  All ranks pass models of one shape and configuration. */
int vrx_comm_bcast_model(vrx_comm* c, vrx_model* m, int root);

/* ---- restart initialisation ------------------------------------------------------------
 * Every restart's initial ID_prob / GT_prob comes from NumPy's legacy global stream
 * (np.random.rand in vireo_model.py:98,103, one Vireo per restart in vireo_wrap.py:66-71).
 * Continue that stream in C: write the next n doubles of RandomState.random_sample() to
 * `out`, or (out == NULL) skip them, advancing the MT19937 state of np.random.get_state()
 * (key[624], pos) in place.  Host only; no GPU needed. */
int vrx_mt19937_random_sample(uint32_t* key624, int32_t* pos, double* out, int64_t n);
/* Skip n doubles of the same stream.  A rank of the restart shard (vireo_wrap.py:66-71: restart i
 * on rank i % world) must pass every other rank's draws; far skips are a JUMP of the generator --
 * the polynomial x^(624 R) mod phi of its GF(2) transition matrix applied to the state, cached per
 * skip length, ~1 ms whatever the distance -- instead of R regenerations.  jump: 1 = jump
 * whenever the skip spans >= 3 regenerations, 0 = always step (the specification the jump is
 * tested against, bit for bit), -1 = the library's threshold (what out == NULL above uses). */
int vrx_mt19937_skip(uint32_t* key624, int32_t* pos, int64_t n, int32_t jump);
/* np.sum() of a contiguous float32 array, bit for bit (NumPy's pairwise summation per 8192-element
 * iterator chunk).  vrx_problem_binom_const adds the float32 terms of get_binom_coeff
 * (vireo_base.py:7-22) with it, like vireo_model.py:313 does with np.sum.  Host only. */
int vrx_np_sum_f32(const float* a, int64_t n, float* out);

/* ---- MatrixMarket input (f4) -----------------------------------------------------------
 * cellSNP.tag.{AD,DP}.mtx and the vartrix matrices, which the reference reads with
 * scipy.io.mmread (io_utils.py:57,72-73): a multi-threaded parser of `coordinate`
 * `integer` / `real` (integral values) / `pattern`, `general` files.  vrx_mtx_header returns
 * the shape and entry count; vrx_mtx_read fills caller-allocated COO arrays (0-based, file
 * order, duplicates kept).  n_threads <= 0: all cores (at most 64).  Host only. */
int vrx_mtx_header(const char* path, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
/* AD and DP (canonical CSC, any of the dtypes the reference's loaders produce) -> the union
 * pattern with an (ad, dp) pair per entry, the input of vrx_problem_create: what
 * `BD = DP - AD` and the separate AD / DP products of the reference (vireo_model.py:167-170)
 * are replaced by.  Two passes: with rowidx == NULL the per-column entry counts go to
 * colptr[1..n_cell]; the caller accumulates them and calls again to fill.  *_ptr64 / *_idx64:
 * the index arrays are int64 (else int32); *_kind: counts are 0 int32, 1 int64, 2 float64.
 * Host only, multi-threaded. */
int vrx_merge_counts(int64_t n_var, int64_t n_cell, const void* ad_ptr, const void* ad_idx,
                     const void* ad_dat, int ad_ptr64, int ad_idx64, int ad_kind,
                     const void* dp_ptr, const void* dp_idx, const void* dp_dat, int dp_ptr64,
                     int dp_idx64, int dp_kind, int64_t* colptr, int32_t* rowidx, int32_t* ad,
                     int32_t* dp, int n_threads);
int vrx_mtx_read(const char* path, int64_t nnz, int32_t* row, int32_t* col, int32_t* val,
                 int n_threads);
/* The COO arrays of vrx_mtx_read -> CSC: `mmread(...).tocsc()` of read_cellSNP / read_vartrix
 * (io_utils.py:57,72-73; SciPy's single-threaded coo_tocsr) as a stable counting sort by column
 * on all cores.  colptr [n_cols + 1], rowidx / data [nnz] (data int64 like mmread's).
 * *canonical = 1 when every column's rows come out strictly increasing (no duplicates, file was
 * row-major: what cellSNP writes); 0: the caller must sort / sum duplicates (SciPy does).
 * Host only. */
int vrx_coo_to_csc(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* row,
                   const int32_t* col, const int32_t* val, int64_t* colptr, int32_t* rowidx,
                   int64_t* data, int32_t* canonical, int n_threads);
/* The inverse of vrx_mtx_read: a `coordinate integer general` file from 0-based COO arrays, in
 * the given order (the format of cellSNP's cellSNP.tag.{AD,DP}.mtx that read_cellSNP loads,
 * io_utils.py:57; the reference itself never writes one).  Multi-threaded formatting; used by
 * bench.py's end-to-end leg and the parser's round-trip test.  Host only. */
int vrx_mtx_write(const char* path, int64_t n_rows, int64_t n_cols, int64_t nnz,
                  const int32_t* row, const int32_t* col, const int32_t* val);

/* ---- text writers of the command (host only) ----------------------------------------------
 * vrx_write_table: prob_singlet.tsv / prob_doublet.tsv of write_donor_id (io_utils.py:147-170):
 * `header`, then per row its label and `cols` numbers in the printf format `fmt` ("%.2e"), tab
 * separated.  vrx_write_vcf_records: the donor genotype VCF of write_VCF (vcf_utils.py:234-296)
 * with the tags GT:AD:DP:PL -- `head`, then per variant its prefix (fixed columns + FORMAT) and
 * per sample <0/0|1/0|1/1>:AD:DP:PL,PL,PL from integer arrays.  gz != 0 writes gzip (one member
 * per chunk of rows).  Chunks are formatted and deflated on several threads. */
int vrx_write_table(const char* path, const char* header, const char* names,
                    const int64_t* name_off /* rows + 1 */, const double* table, int64_t rows,
                    int64_t cols, const char* fmt, int32_t gz);
int vrx_write_vcf_records(const char* path, const char* head, const char* prefix,
                          const int64_t* prefix_off /* n_var + 1 */, const int8_t* call,
                          const int64_t* ad, const int64_t* dp, const int64_t* pl /* [..][3] */,
                          int64_t n_var, int64_t n_sample, int32_t gz);

/* ---- the stop rule of the fit loops (csrc/vrx_stop.h), test infrastructure ---------------------
 * Every fit loop of the library judges its iterations with vrx_stop_judge, in the form of its
 * reference loop (vireo_model.py:266-274, bmm_model.py:190-199, vireo_bulk.py:97-105 =
 * vireo_doublet.py:173-181).  vrx_stop_verdicts runs the device compile of that judge on n rows,
 * one lane per row: rows_i [n][4] = (form, it, min_iter, max_iter), rows_d [n][3] = (eps,
 * X[it - 1] as the trace holds it, X[it]); verdict [n] = 0 continue, 1 warn "decreased",
 * 2 warn "did not converge", 3 stop; prev [n] = the value X[it - 1] was taken to have (it = 0:
 * 0, or X[it] when max_iter = 1, like Python's X[-1] of np.zeros(max_iter)). */
int vrx_stop_verdicts(int device, int64_t n, const int32_t* rows_i, const double* rows_d,
                      int32_t* verdict, double* prev);

#ifdef __cplusplus
}
#endif
#endif /* VIREO_HIP_H */
