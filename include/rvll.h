/*
 * rvll.h — C-ABI of the MI355X-native RV log-likelihood engine ("rvll").
 *
 * This is the drop-in boundary for the one hot path of nicochunger/evidence:
 * the per-live-point Keplerian RV forward model + Gaussian log-likelihood and
 * the unit-cube -> theta prior transform.  Everything here is extern "C",
 * plain pointers and sizes; the caller owns every host buffer, the library
 * owns device memory behind an opaque handle.  One handle = one device + its
 * own HIP streams.  A handle is not thread-safe; distinct handles are
 * independent.
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference checkout):
 *
 *   rvll_create              evidence/rvmodel/__init__.py:23-57,94-154
 *                            (BaseModel/RVModel.__init__: concatenated epoch
 *                            table, instrument ids, planet count, model flags)
 *   rvll_loglike_batch       evidence/rvmodel/__init__.py:157-219 (log_likelihood)
 *                            -> :343-385 (kep_rv) -> :388-463 (modelk)
 *                            -> :466-494 (true_anomaly) -> rvmodel/trueanomaly.c:8-41
 *                            -> :222-273 (drift) -> :59-80 (logL)
 *                            (fp64: the planets' Keplerian quotients of :463 and
 *                            the res^2 / (2 var) of :80 are pooled over one
 *                            denominator and divided once per (point, epoch);
 *                            the constants K e cos w of :463 are summed per
 *                            point: rvll_math.h ItemPool, rvll_tile.h eval_item)
 *                            i.e. it is the batched form of the existing FFI
 *                            `int trueanomaly(double*,int,double,double*,int,double)`
 *                            (rvmodel/trueanomaly.h:4) fused with its caller.
 *   rvll_set_priors /
 *   rvll_prior_batch         evidence/priors.py:22-460 (.ppf of every
 *                            distribution) as called from
 *                            evidence/polychord/__init__.py:130-162 and
 *                            evidence/ultranest/__init__.py:125-137
 *   rvll_prior_loglike_batch prior(cube) followed by loglike(theta), one launch
 *   rvll_comm_* / rvll_allgather_logl
 *                            replaces the MPI fan-out owned by the third-party
 *                            samplers (evidence/polychord/__init__.py:21-29,
 *                            176-199) with one RCCL all-gather of per-shard log-L
 *
 * Error convention: every function returns 0 on success or a negative
 * RVLL_E_* code; rvll_last_error() returns a human-readable message for the
 * calling thread's last failure.  Model-level conditions are NOT errors and
 * follow the reference: an invalid orbit (ecc > 1 in the secos/sesin or
 * ecos/esin parametrisation) gives log-L = -1e30
 * (evidence/rvmodel/__init__.py:198-203,430-431,438-439).
 */
#ifndef RVLL_H
#define RVLL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVLL_VERSION_MAJOR 0
#define RVLL_VERSION_MINOR 8   /* 0.2: rvll_slice_walk takes walker_base; RVLL_FLAG_WANDERED; resident live set
                                  0.3: rvll_slice_walk_runs
                                  0.4: rvll_cluster_runs
                                  0.5: rvll_live_runs_* (resident ensemble)
                                  0.6: rvll_live_runs_step_clustered, rvll_live_runs_clusters
                                  0.7: rvll_shrinkage_replicates
                                  0.8: rvll_live_births, rvll_live_runs_births, rvll_insertion_indexes;
                                       additions within 0.8 (new symbols only, no signature changed):
                                       rvll_slice_walk_runs_steps, rvll_walk_distances_runs, rvll_live_runs_step_steps,
                                       rvll_set_walk_proposal (RVLL_PROPOSAL_CHORD / _STEPOUT),
                                       rvll_merge_runs, rvll_merge_replicates (rvll_merge_timing),
                                       rvll_posterior_replicates (rvll_posterior_timing),
                                       rvll_fip_replicates (rvll_fip_merged_timing),
                                       rvll_marginal_replicates (rvll_marginal_timing),
                                       rvll_region_draw_runs, rvll_region_tile_rows,
                                       rvll_draw_replicates (rvll_draw_timing), rvll_kep_rv_bands,
                                       rvll_pointwise_replicates (rvll_pointwise_timing), rvll_pointwise_slab_rows,
                                       rvll_prior_logpdf_batch (rvll_prior_density, rvll_density_timing) */

/* ---- error codes ------------------------------------------------------ */
#define RVLL_OK             0
#define RVLL_E_INVALID     -1   /* bad argument / inconsistent layout        */
#define RVLL_E_NODEVICE    -2   /* no HIP device, or device index invalid    */
#define RVLL_E_HIP         -3   /* a HIP runtime call failed                 */
#define RVLL_E_NOMEM       -4   /* host or device allocation failed          */
#define RVLL_E_NOPRIORS    -5   /* prior transform requested before set_priors */
#define RVLL_E_RCCL        -6   /* RCCL missing or a collective failed       */
#define RVLL_E_UNSUPPORTED -7   /* feature not available in this build       */

/* ---- per-point flag bits written by the log-L kernels ------------------ */
#define RVLL_FLAG_INVALID_ORBIT  1  /* ecc>1 in a derived parametrisation -> logL=-1e30 */
#define RVLL_FLAG_NONCONVERGED   2  /* a Kepler solve hit itmax (trueanomaly.c:32-33 path) */
#define RVLL_FLAG_WANDERED       4  /* a Kepler solve of this point took more than 8 Newton steps.  The reference's
                                     * iteration (Newton from E = M, stop at |dE| <= 1e-4, trueanomaly.c:17-33) only does
                                     * that next to a zero of f' = 1 - e cos E at e >= ~0.97, where it is thrown far out
                                     * and wanders back: where it then stops depends on the last bit of sin / cos, so the
                                     * reference's own log-L there is only defined to ~1e-9 relative (measured on the
                                     * oracle with its libm nudged by one ulp).  The contract: every point
                                     * WITHOUT this bit agrees with the reference to <= 1e-10; a point with it to what
                                     * the reference agrees with itself.  SURVEY 0.3 / 5: the per-point flag the
                                     * reference lacks (it ignores the solver's return code, rvmodel/__init__.py:488-492).
                                     * With RVLL_FLAG_INVALID_ORBIT set, only that bit is reported.
                                     * Such a solve is done again with correctly rounded sin / cos (rvll_set_wander_exact).
                                     * With 9 < itmax that redo can run out of steps where the first try converged: the
                                     * planet's array is then abandoned from the earliest epoch at which EITHER try ran out
                                     * (RVLL_FLAG_NONCONVERGED is set) — a function of the point alone, whatever the kernel
                                     * form and tiling. */

/* ---- parameter slot: where a model scalar comes from ------------------- */
/* idx >= 0 : free parameter, value = theta[idx]   (theta ordered as sorted(parnames),
 *            evidence/rvmodel/__init__.py:43)
 * idx <  0 : fixed parameter, value = val         (fixedpardict)              */
typedef struct rvll_slot {
    int32_t idx;
    int32_t reserved;
    double  val;
} rvll_slot;

/* parametrisation choices of modelk (evidence/rvmodel/__init__.py:412-456) */
enum { RVLL_K_K1 = 0, RVLL_K_LOGK1 = 1 };                 /* :412-415 */
enum { RVLL_P_PERIOD = 0, RVLL_P_LOGPERIOD = 1 };         /* :417-420 */
enum { RVLL_ECC_DIRECT = 0,                               /* ecc, omega      :441-447 */
       RVLL_ECC_SECOS_SESIN = 1,                          /* sqrt(e)cos/sin  :425-431 */
       RVLL_ECC_ECOS_ESIN = 2 };                          /* e cos/sin       :433-439 */
enum { RVLL_ANOM_MA0 = 0, RVLL_ANOM_ML0 = 1 };            /* :449-454 */

typedef struct rvll_planet {
    int32_t   k_kind;
    int32_t   p_kind;
    int32_t   ecc_kind;
    int32_t   anom_kind;
    rvll_slot k;        /* k1 | logk1                          */
    rvll_slot p;        /* period | logperiod                  */
    rvll_slot e1;       /* ecc   | secos | ecos                */
    rvll_slot e2;       /* omega | sesin | esin                */
    rvll_slot anom;     /* ma0 | ml0                           */
    rvll_slot epoch;    /* planet{n}_epoch                     */
} rvll_planet;

typedef struct rvll_inst {
    rvll_slot offset;   /* {inst}_offset  (rvmodel:187)                       */
    rvll_slot jitter;   /* {inst}_jitter  (rvmodel:189-190); unused if !has_jitter */
} rvll_inst;

/* RVLL_PREC_FP64  : everything fp64, the reference's arithmetic (parity <= 1e-10).
 * RVLL_PREC_MIXED : mean anomaly and its reduction to [-pi,pi] in fp64 (|M| reaches 1e4 rad, which
 *                   fp32 cannot hold), Newton iteration + Keplerian in fp32, residual / chi^2 /
 *                   accumulation in fp64.  NOT parity with the reference: BASELINE.json configs[4]
 *                   tolerance sweep (~1e-7 relative on log-L).
 * RVLL_PREC_FP32  : as MIXED, with the per-epoch residual and chi^2 term in fp32 as well (the sum
 *                   over epochs stays fp64).                                                     */
enum { RVLL_PREC_FP64 = 0, RVLL_PREC_MIXED = 1, RVLL_PREC_FP32 = 2 };

typedef struct rvll_layout {
    int32_t struct_size;       /* = sizeof(rvll_layout), ABI check            */
    int32_t ndim;              /* D = number of free parameters               */
    int32_t nplanets;          /* rvmodel:122-124                             */
    int32_t ninst;             /* number of instruments (datadict keys)       */
    int32_t has_jitter;        /* rvmodel:138-139                             */
    int32_t has_drift;         /* rvmodel:128-129                             */
    int32_t tref_from_data;    /* 1: tref = time[0] (rvmodel:259-260)         */
    int32_t nlinpar;           /* number of linear-activity series (rvmodel:210-212) */
    rvll_slot drift[4];        /* lin, quad, cub, quar (rvmodel:246-253)      */
    rvll_slot tref;            /* drift_tref (rvmodel:257-258)                */
    const rvll_planet* planets;   /* [nplanets]                               */
    const rvll_inst*   insts;     /* [ninst]                                  */
    const rvll_slot*   linpar;    /* [nlinpar] coefficients linpar_X          */
    double  tol;               /* Newton stop rule, 1e-4 (rvmodel:466)        */
    int32_t itmax;             /* 10000 (rvmodel:491)                         */
    int32_t precision;         /* RVLL_PREC_*                                 */
} rvll_layout;

/* ---- priors ------------------------------------------------------------ */
/* Kinds follow the names exported by evidence/priors.py:429-467.            */
enum {
    RVLL_PRIOR_UNIFORM = 0,          /* priors.py:41-42   args xmin,xmax     */
    RVLL_PRIOR_JEFFREYS = 1,         /* :62-63            xmin,xmax          */
    RVLL_PRIOR_MODJEFFREYS = 2,      /* :82-83            x0,xmax            */
    RVLL_PRIOR_UNIFORMFREQUENCY = 3, /* :100-101          xmin,xmax          */
    RVLL_PRIOR_NORMAL = 4,           /* :436 stats.norm   loc,scale          */
    RVLL_PRIOR_LOGNORMAL = 5,        /* :437 stats.lognorm s,loc,scale       */
    RVLL_PRIOR_TRUNCRAYLEIGH = 6,    /* :249-252          sigma,xmax         */
    RVLL_PRIOR_TABLE = 7,            /* piecewise-linear inverse CDF on a host-built
                                        grid: Binormal :118-124, AsymmetricNormal
                                        :195-202, TruncatedUNormal :223-228,
                                        PowerLaw :282-287, DoublePowerLaw :321-326,
                                        Sine :349-354, Log10Normal :138-144.
                                        args: lo,hi (values returned at q==0 / q==1),
                                        flags                                 */
    RVLL_PRIOR_BETA = 8,             /* :397-398 stats.beta.ppf   a,b         */
    RVLL_PRIOR_GAMMA = 9,            /* :424-425 stats.gamma.ppf  alpha,beta  */
    RVLL_PRIOR_ALPHA = 10,           /* :375-376 stats.alpha.ppf  a           */
    RVLL_PRIOR_SORTED_UNIFORM = 11,  /* priors.py:462-467 (pypolychord)  a,b  */
    RVLL_PRIOR_SORTED_LOGUNIFORM = 12,
    RVLL_PRIOR__COUNT
};

#define RVLL_PRIOR_NARGS 6
typedef struct rvll_prior {
    int32_t kind;
    int32_t group;             /* sorted priors: members of one group share an id >= 0 */
    double  args[RVLL_PRIOR_NARGS];
    const double* table_cdf;   /* RVLL_PRIOR_TABLE: sorted knots  [table_n]  */
    const double* table_x;     /*                   values         [table_n]  */
    int32_t table_n;
    int32_t table_post;        /* 0: y ; 1: 10**y  (Log10Normal)              */
} rvll_prior;

/* ---- timing report of the device-resident benchmark -------------------- */
typedef struct rvll_timing {
    double kernel_ms_mean;     /* mean HIP-event time per launch             */
    double kernel_ms_min;
    double kernel_ms_median;
    double total_ms;           /* first launch -> last launch complete       */
    int64_t evals;             /* live points evaluated in total             */
    int32_t launches;
    int32_t points_per_block;  /* launch geometry actually used              */
    int32_t blocks;
    int32_t threads;
} rvll_timing;

typedef struct rvll_handle rvll_handle;

/* ---- lifecycle ---------------------------------------------------------- */
/* Upload the concatenated epoch table once.  Arrays are in the reference's
 * concatenation order (instrument by instrument, evidence/rvmodel/__init__.py:50-55),
 * NOT time-sorted.  inst[j] in [0,ninst).  linpar_series is [nlinpar][Ne]
 * row-major or NULL.  device < 0 selects the current HIP device.            */
int rvll_create(const rvll_layout* layout,
                const double* time, const double* vrad, const double* svrad,
                const int32_t* inst, int32_t n_epochs,
                const double* linpar_series,
                int32_t device, rvll_handle** out);
int rvll_destroy(rvll_handle* h);

/* ---- priors -------------------------------------------------------------- */
int rvll_set_priors(rvll_handle* h, const rvll_prior* priors, int32_t ndim);
/* Beta and Gamma quantiles (scipy.stats.beta/gamma.ppf, evidence/priors.py:397-398, 424-425) have no closed
 * form: rvll_set_priors lets the device tabulate each one once and MEASURES the table's quintic interpolant
 * against the full iterative solver.  max_err = that measured error (relative, in the interpolation
 * coordinate; NaN for parameters without such a table); direct = 1 if it is small enough that elements are
 * evaluated by interpolation alone, 0 if every element still runs a Newton step on the incomplete
 * beta/gamma function.  Diagnostics only.                                                               */
int rvll_prior_table_info(rvll_handle* h, int32_t dim, double* max_err, int32_t* direct);

/* ---- the hot calls (host buffers in, host buffers out) ------------------- */
/* theta: [B, D] row-major.  logL: [B].  flags: [B] or NULL.                  */
int rvll_loglike_batch(rvll_handle* h, const double* theta, int64_t B,
                       double* logL, int32_t* flags);
/* cube: [B, D] in [0,1].  theta: [B, D].                                     */
int rvll_prior_batch(rvll_handle* h, const double* cube, int64_t B, double* theta);
/* fused: one H2D, prior + log-L launches back to back, one D2H.
 * From 24 MB of rows on (165565 points at 19 parameters) the batch is streamed: chunks of 16384 rows through pinned staging blocks, uploads, kernels and
 * downloads on three streams, and the copies between the caller's (pageable) arrays and the blocks on worker
 * threads of the library — 2 to 4, RVLL_COPY_THREADS overrides; started by the first such call of a handle, asleep
 * between calls, joined by rvll_destroy.  The caller's arrays are only touched between entry and return.           */
int rvll_prior_loglike_batch(rvll_handle* h, const double* cube, int64_t B,
                             double* theta_out, double* logL, int32_t* flags);

/* ---- sampler proposal step on the device ---------------------------------------------------------------- */
/* The callers of the path: nested sampling replaces its worst points by new points drawn
 * from the prior inside logL > lstar.  The reference leaves that to UltraNest's region slice sampler
 * (evidence/ultranest/__init__.py:159-175: RegionSliceSampler, nsteps moves per new point, circular omega / ml0);
 * evidence_amd/nested.py does the same with batched callbacks.  This entry point runs the whole walk on the GPU:
 * K walkers start at cube[K, ndim] (theta / logl hold their transformed parameters and log-L, all above lstar)
 * and take nsteps hit-and-run slice moves each: direction = chol * normal / norm (chol: [ndim, ndim] row-major
 * lower-triangular factor of the live points' covariance), chord limited by the unit-cube walls (wrapped[k] != 0:
 * circular parameter, half a turn), candidate = uniform point of the chord -> prior transform -> log-L, accepted
 * if logL > lstar, else the chord shrinks towards the current point (at most max_rounds candidates per move).
 * In/out buffers return the end points; *ncalls = likelihood evaluations spent.  Deterministic for a given
 * seed: the random numbers are counter-based on (seed, walker_base + row, move, draw), so a rank that walks rows
 * [lo, hi) of a larger set with walker_base = lo gets exactly what the unsharded walk gives those rows — a run does
 * not depend on how many GPUs share it.  Needs rvll_set_priors.                                              */
int rvll_slice_walk(rvll_handle* h, double* cube, double* theta, double* logl, int64_t K, double lstar,
                    const double* chol, const int32_t* wrapped /*[ndim] or NULL*/, int32_t nsteps,
                    int32_t max_rounds, uint64_t seed, int64_t walker_base, int64_t* ncalls);
/* The walks of R independent runs of one model in ONE walk (the repeats of a FIP workflow: the same model sampled R times
 * with different seeds, ln Z and p(k | y) taken over the runs).  One run's walk is a few hundred walkers — a few dozen
 * workgroups on a chip that holds thousands, its time set by the latency of a chain of dependent moves; the walkers of R runs
 * walk side by side for about the cost of one.  Walkers are grouped by run: rows run_start[r] .. run_start[r + 1] of
 * cube / theta / logl [K, ndim], [K, ndim], [K] belong to run r (K = run_start[R], run_start[0] = 0; empty runs are allowed).
 * Run r has its own lstar[r], whitening factor chol[r] ([R, ndim, ndim] row-major lower-triangular) and seed[r]; wrapped,
 * nsteps and max_rounds are common.  End points, theta, log-L and ncalls[r] of run r are bit for bit those of
 * rvll_slice_walk(rows of run r, lstar[r], chol[r], wrapped, nsteps, max_rounds, seed[r], walker_base = 0): the walker at row
 * run_start[r] + i draws from the counters (seed[r], i, move, draw), and its calls are counted per walker in every form the
 * walk takes (the single-kernel forms and their parts, the rounds form, the full-solver finish of walkers the slim prior
 * stage deferred), then summed by run.  ncalls [R] may be NULL.  The measurement switch RVLL_WALK_ROWS (the rows forms) has
 * no run mode: with it set this returns RVLL_E_UNSUPPORTED.  rvll_slice_walk_evaluated / _rounds report on this walk as on
 * rvll_slice_walk's.  Needs rvll_set_priors.                                                                                */
int rvll_slice_walk_runs(rvll_handle* h, double* cube, double* theta, double* logl /*[K, ndim], [K, ndim], [K]*/,
                         const int64_t* run_start /*[R + 1]*/, int32_t R,
                         const double* lstar /*[R]*/, const double* chol /*[R, ndim, ndim]*/, const uint64_t* seed /*[R]*/,
                         const int32_t* wrapped /*[ndim] or NULL*/, int32_t nsteps, int32_t max_rounds,
                         int64_t* ncalls /*[R] out*/);
/* rvll_slice_walk_runs with a step count per run: run r makes nsteps[r] moves (0 <= nsteps[r] < 2^18), and its rows, theta,
 * log-L and ncalls[r] are bit for bit those of rvll_slice_walk(rows of run r, ..., nsteps[r], ...).  A uniform table is
 * rvll_slice_walk_runs itself; otherwise every row stops after its run's count in the single-kernel forms (the rounds form,
 * whose direction table holds the same number of moves for every walker, is not taken).  For the step-count adaptation
 * of evidence_amd/adapt.py.                                                                                  */
int rvll_slice_walk_runs_steps(rvll_handle* h, double* cube, double* theta, double* logl /*[K, ndim], [K, ndim], [K]*/,
                               const int64_t* run_start /*[R + 1]*/, int32_t R,
                               const double* lstar /*[R]*/, const double* chol /*[R, ndim, ndim]*/, const uint64_t* seed /*[R]*/,
                               const int32_t* wrapped /*[ndim] or NULL*/, const int32_t* nsteps /*[R]*/, int32_t max_rounds,
                               int64_t* ncalls /*[R] out*/);
/* The distances of the step-count adaptation (definition: DESIGN §4h, evidence_amd/adapt.py).  Rows group_start[g] ..
 * group_start[g + 1] of survivors [N, ndim] (unit-cube rows) are the members of group g, whose lower-triangular factor is
 * factors[g] ([G, ndim, ndim] row-major); walker k went from starts[k] to ends[k] ([K, ndim]) in group walker_group[k].
 * Out: pair_out[g], the mean over the unordered pairs of group g of dist_g (NaN below two members), and move_out[k] =
 * dist_g(starts[k], ends[k]) — with dist_g the length of the solution of L_g z = delta by forward substitution, delta the
 * row difference (minimum image on wrapped dimensions), every operation IEEE-rounded on its own.  move_out and every pair
 * distance are the definition's bits; a group's pair sum has a fixed order of its own (pair_out does not depend on the other
 * groups of the call).  RVLL_E_INVALID: group_start not rising from 0 to N, walker_group out of range, a required pointer
 * NULL; RVLL_E_UNSUPPORTED: ndim above 64.  Needs no priors.                                                            */
int rvll_walk_distances_runs(rvll_handle* h, const double* survivors /*[N, ndim]*/, const int64_t* group_start /*[G + 1]*/,
                             int32_t G, const double* factors /*[G, ndim, ndim]*/, const int32_t* wrapped /*[ndim] or NULL*/,
                             const double* starts /*[K, ndim]*/, const double* ends /*[K, ndim]*/,
                             const int32_t* walker_group /*[K]*/, int64_t K, double* pair_out /*[G]*/, double* move_out /*[K]*/);
/* MLFriends clustering of R independent row sets in one call (definition: DESIGN §4e).  Rows run_start[r] .. run_start[r+1]
 * of cube belong to run r; scale [R, ndim] is each run's metric (1 / per-dimension spread); wrapped [ndim] may be NULL;
 * 0 <= nboot <= 32; seeds [R].  Out: labels [run_start[R]] (cluster of each row inside its run, 0-based, by smallest row),
 * nclusters [R], radius2 [R].  The result does not depend on scheduling: it is bit for bit that of the numpy definition
 * (evidence_amd/clustering.py).  An empty run gets nclusters 0 and radius2 0.  RVLL_E_INVALID: nboot outside [0, 32],
 * run_start not rising from 0, a scale that is not finite and positive, a required pointer NULL; RVLL_E_UNSUPPORTED: ndim
 * above 64.  Needs no priors.                                                                                               */
/* The resident ensemble's step with one step count per listed run (rvll_live_runs_step, or with clustered != 0
 * rvll_live_runs_step_clustered with nboot / boot_seeds / nclusters, otherwise the same arguments): run a walks nsteps[a] moves.
 * move / pair [A kdead] (either may be NULL) receive, per walker in the order of ranks, the step-count adaptation's distances
 * (DESIGN §4h): move = dist_g(start, end) and pair = pair_g of the walker's group g (the run, or the run's cluster its start row
 * is in), computed on the device from the live rows after the walk, with no host synchronisation of their own.  A uniform
 * table with move and pair NULL is rvll_live_runs_step / _clustered bit for bit.  nclusters is only written when clustered. */
int rvll_live_runs_step_steps(rvll_handle* h, const int32_t* runs /*[A]*/, int32_t A, int64_t kdead, const int32_t* ranks /*[A kdead]*/,
                              const double* lstar /*[A]*/, const int32_t* wrapped, const int32_t* nsteps /*[A]*/, int32_t max_rounds,
                              const uint64_t* seeds /*[A]*/, int32_t clustered, int32_t nboot, const uint64_t* boot_seeds /*[A] or NULL*/,
                              int64_t* ncalls /*[A]*/, double* logl_new /*[A kdead]*/, int32_t* nclusters /*[A] or NULL*/,
                              double* move /*[A kdead] or NULL*/, double* pair /*[A kdead] or NULL*/);
int rvll_cluster_runs(rvll_handle* h, const double* cube /*[N, ndim]*/, const int64_t* run_start /*[R + 1]*/, int64_t R,
                      const double* scale, const int32_t* wrapped, int nboot, const uint64_t* seeds,
                      int32_t* labels, int32_t* nclusters, double* radius2);
/* A walker's moves are a chain of dependent evaluations; when walkers of a workgroup have finished, the free slots of
 * its tile evaluate, for the walkers that are left, up to max_ahead candidates of the current move per iteration:
 * candidate r+1 is the one the walker draws if candidate r is rejected (the shrunk bracket is known in advance), and
 * the results are consumed in order — so end points, log-L and *ncalls are those of the one-candidate-per-iteration
 * walk, bit for bit; only the number of iterations drops.  Default 4; 1 switches it off.
 * rvll_slice_walk_evaluated: tile slots the last rvll_slice_walk evaluated (>= its ncalls: speculative candidates
 * that went unused are work done, not likelihood calls of the sampler).                                          */
int rvll_set_walk_speculation(rvll_handle* h, int32_t max_ahead);
/* The proposal of every walk on the handle from now on — rvll_slice_walk*, rvll_live_step, rvll_live_runs_step* with and
 * without clustering.  RVLL_PROPOSAL_CHORD (the default): hit-and-run, each move shrinking the whole unit-cube
 * chord along a random unit direction towards the walker.  RVLL_PROPOSAL_STEPOUT: PolyChord-style slice sampling — move m
 * goes along L q_{m mod ndim}, q the vectors of a random orthonormal basis drawn anew every ndim moves (modified
 * Gram-Schmidt), t in whitened units; a bracket `width` wide at a uniform offset around the walker, cut by the cube's walls
 * (wrapped parameters set no limit), steps out by `width` at each end inside the slice (right end first), then shrinks as
 * the chord walk does.  Expansions and shrink candidates count together against max_rounds.  Counter-based draws name the
 * walker, so sharding (walker_base), run mode and the queue give the same bits as with the chord walk.  A stepout walk
 * takes the single-kernel forms only (rvll_slice_walk_rounds reports 0; RVLL_WALK_ROWS -> RVLL_E_UNSUPPORTED), at most 64
 * parameters, and per-walker-slot scratch of ndim^2 doubles.  RVLL_E_INVALID: an unknown kind, a width that is not
 * positive and finite, or (at the walk) a stepout walk in which every parameter is wrapped.                       */
#define RVLL_PROPOSAL_CHORD   0
#define RVLL_PROPOSAL_STEPOUT 1
int rvll_set_walk_proposal(rvll_handle* h, int32_t kind, double width);
int rvll_slice_walk_evaluated(rvll_handle* h, int64_t* evaluated);
/* Diagnostic build only (make -C evidence_amd/csrc walktrace; all zeros otherwise): where the workgroups of the last
 * rvll_slice_walk spent their time — 100 MHz ticks summed over workgroups for [0] directions + chord limits,
 * [1] candidates, [2] prior transform + log-L tile, [3] accept / copy / bookkeeping; [4] = number of workgroups;
 * [5] = the longest workgroup life, in ticks. */
int rvll_slice_walk_phases(rvll_handle* h, uint64_t out[6]);
/* Which form the last rvll_slice_walk / rvll_live_step took: *rounds = the number of rounds of the ROUNDS form (a round = one
 * launch that proposes and accepts for a group of walkers + one launch of the batch log-L kernel over the group's candidates,
 * no host synchronisation in between; the default wherever every Beta / Gamma prior has a verified table), 0 = one of the
 * single-kernel forms walked (RVLL_WALK_ROUNDS=0, or one of their switches).  Same results either way, bit for bit. */
int rvll_slice_walk_rounds(rvll_handle* h, int32_t* rounds);

/* ---- nested sampling with the live points resident on the device ----------------------------------------------- */
/* rvll_slice_walk above takes and returns its walkers through host buffers; a sampler built on it ships three row sets
 * each way per iteration (start points up, end points down) and gathers / scatters them on the host — a fifth of the
 * end-to-end time of evidence_amd/nested.py at 32768 live points.  With these entry points the live set (unit-cube rows,
 * theta, log-L) and the points that died stay in HBM for the whole run; per iteration the host sends indices and reads
 * back log-L — what it needs for the sort and the evidence sum (the part of evidence/ultranest/__init__.py:165-185 that is
 * the sampler's bookkeeping, not its likelihood calls).
 *
 * rvll_live_init   N unit-cube rows -> prior transform -> log-L (as rvll_prior_loglike_batch); the three arrays stay resident;
 *                  logl_out [N] (may be NULL).  Starts a new run (the dead store is emptied).
 * rvll_live_step   one iteration: order [N] = the live rows by ascending log-L.  The rows order[0 .. kdead) die — their
 *                  theta and log-L are appended to the dead store, in that order; kdead walkers start from rows
 *                  start[0 .. kdead) (the sampler draws them among the survivors order[kdead .. N)), walk nsteps moves
 *                  inside logL > lstar exactly as rvll_slice_walk does (same kernels, same counter-based random numbers:
 *                  walker i is row walker_base + i), and their end points replace the dead rows (walker i -> row
 *                  order[i]).  chol: the whitening factor [ndim, ndim], or NULL to have the covariance of the surviving
 *                  rows summed on the device (two passes, fixed order) and factored by the library; chol_out (may be
 *                  NULL) receives the factor that was used.  logl_new [kdead]: the new log-L of rows order[0 .. kdead).
 * rvll_live_sort   (round 4) the order itself, on the device: the live rows by ascending log-L (stable: ties by row, as
 *                  numpy's stable argsort) are sorted there and stay there; dead_logl [kdead] receives the log-L of the kdead
 *                  lowest in that order (the sampler's evidence sums need them), *lstar the kdead-th lowest, *max_logl the
 *                  highest.  The rvll_live_step that follows is then called with order = NULL, and its start [kdead] are
 *                  RANKS among the survivors (0 .. N - kdead - 1; the sampler's random draw): walker i starts from the row
 *                  of rank start[i].  A sampler then mirrors nothing per live point on the host: per iteration kdead ranks go
 *                  up, 2 kdead log-L values come down (0.6 ms of host sort and 128 KB of order per iteration at 32768 live
 *                  points before).
 * rvll_live_get    the live set as it stands (any pointer may be NULL).
 * rvll_live_dead   *n_dead in: capacity of theta [*, ndim] / logl [*] in rows (ignored when both are NULL);
 *                  out: rows in the dead store.  Rows are in the order they died.                                     */
int rvll_live_init(rvll_handle* h, const double* cube /*[N, ndim]*/, int64_t N, double* logl_out /*[N] or NULL*/);
int rvll_live_step(rvll_handle* h, const int32_t* order /*[N], or NULL after rvll_live_sort*/, int64_t kdead, const int32_t* start /*[kdead]*/,
                   double lstar, const double* chol /*[ndim, ndim] or NULL*/, const int32_t* wrapped /*[ndim] or NULL*/,
                   int32_t nsteps, int32_t max_rounds, uint64_t seed, int64_t walker_base, int64_t* ncalls,
                   double* logl_new /*[kdead]*/, double* chol_out /*[ndim, ndim] or NULL*/);
int rvll_live_sort(rvll_handle* h, int64_t kdead, double* dead_logl /*[kdead]*/, double* lstar, double* max_logl);
int rvll_live_get(rvll_handle* h, double* cube, double* theta, double* logl);
int rvll_live_dead(rvll_handle* h, int64_t* n_dead, double* theta, double* logl);
/* The resident ENSEMBLE: R independent nested-sampling runs of n live points each, all resident in one handle, sorted, whitened
 * and walked together (nested.run_nested_ensemble(..., live=model)).  A listed run a of rvll_live_runs_step does
 * exactly what rvll_live_step(order = NULL, chol = NULL, walker_base = 0) after rvll_live_sort does for a handle that holds only
 * that run, bit for bit; the walkers of all listed runs walk in one run-mode walk (as rvll_slice_walk_runs), walker i of run a
 * being row i of run a there.  An ensemble and the one-run live set exclude each other: rvll_live_runs_init empties the one-run
 * state (rvll_live_step / _sort / _get then refuse, rvll_live_dead returns RVLL_E_INVALID while an ensemble is loaded), and
 * rvll_live_init empties the ensemble.
 *
 * rvll_live_runs_init  cube [R n, ndim]: run r is rows r n .. r n + n - 1; prior transform and log-L in one pass; logl_out [R n]
 *                      (may be NULL).  Every run's dead store is emptied.  R >= 1, n >= 2, R n < 2^31.
 * rvll_live_runs_sort  for the A listed runs (runs [A]: distinct, ascending, < R) the stable ascending order of their log-L (ties by
 *                      row, as rvll_live_sort), kept on the device; dead_logl [A, kdead] the kdead lowest of every run in order,
 *                      lstar [A] the kdead-th lowest, max_logl [A] the highest.  1 <= kdead < n.
 * rvll_live_runs_step  follows a rvll_live_runs_sort of the same runs and kdead, with the lstar it returned; ranks [A, kdead] are
 *                      ranks among run a's survivors (0 .. n - kdead - 1); seeds [A]; ncalls [A] (may be NULL) and logl_new
 *                      [A, kdead] out; chol_out [A, ndim, ndim] (may be NULL) receives every run's whitening factor.  The dying rows
 *                      go to their runs' dead stores last: a step that fails (a covariance that is not positive definite, a walk
 *                      that fails) leaves every run as it was.
 * rvll_live_runs_get   run r's live set as it stands (any pointer may be NULL).
 * rvll_live_runs_dead  as rvll_live_dead, for run r: its dead rows in the order they died.
 * Errors: RVLL_E_INVALID (arguments, call order), RVLL_E_NOMEM.                                                            */
int rvll_live_runs_init(rvll_handle* h, const double* cube /*[R n, ndim]*/, int32_t R, int64_t n, double* logl_out /*[R n] or NULL*/);
int rvll_live_runs_sort(rvll_handle* h, const int32_t* runs /*[A]*/, int32_t A, int64_t kdead, double* dead_logl /*[A, kdead]*/,
                        double* lstar /*[A]*/, double* max_logl /*[A]*/);
int rvll_live_runs_step(rvll_handle* h, const int32_t* runs /*[A]*/, int32_t A, int64_t kdead, const int32_t* ranks /*[A, kdead]*/,
                        const double* lstar /*[A]*/, const int32_t* wrapped /*[ndim] or NULL*/, int32_t nsteps, int32_t max_rounds,
                        const uint64_t* seeds /*[A]*/, int64_t* ncalls /*[A] or NULL*/, double* logl_new /*[A, kdead]*/,
                        double* chol_out /*[A, ndim, ndim] or NULL*/);
int rvll_live_runs_get(rvll_handle* h, int32_t run, double* cube, double* theta, double* logl);
int rvll_live_runs_dead(rvll_handle* h, int32_t run, int64_t* n_dead, double* theta, double* logl);
/* The clustered step of the resident ensemble (nested.run_nested_ensemble(..., live=model, clustering=True)).  It
 * follows a rvll_live_runs_sort of the same runs and kdead, takes the arguments of rvll_live_runs_step and makes its checks, and
 * for listed run a, with m = n - kdead survivors (the run's ranks kdead .. n - 1 of the sort):
 *   1. the global covariance and whitening factor exactly as rvll_live_runs_step;
 *   2. the metric scale[d] = 1 / sqrt(cov[d, d] + 1e-14), in double on the host;
 *   3. the survivors, in rank order, clustered as rvll_cluster_runs does with that scale, `wrapped`, nboot (0 .. 32) and
 *      boot_seeds[a] (labels and nclusters[a] bit for bit those of evidence_amd/clustering.py);
 *   4. with nclusters[a] > 1, every cluster of at least 2 ndim rows whitened by the factor of its own rows' covariance (those rows
 *      in rank order, summed as rvll_live_step sums them), every other cluster by the run's global factor;
 *   5. walker i (start rank ranks[a, i]) walks in the group of its start row's cluster: the groups in label order, walkers in
 *      their order inside a group, group c with seed seeds[a] (c = 0) or seeds[a] + c * 0xD1B54A32D192ED03 (mod 2^64), its
 *      cluster's factor and lstar[a], walker j of a group being row j of its run in the run-mode walk — the end points are those
 *      of rvll_slice_walk_runs on the same start rows, groups, factors and seeds;
 *   6. walker i's end point replaces dying row i as in rvll_live_runs_step; logl_new [A, kdead] is in walker order, ncalls [A] (may
 *      be NULL) sums the run's groups, nclusters [A] out.
 * A failed step leaves every run as it was.  All device work: the survivors packed by one gather, the clustering on them, one
 * segmented radix sort for every run's (label, rank) order, one segmented moments pass over all (run, cluster) segments, one walk.
 * Host synchronisations before the walk: 3 (global covariances, labels, cluster covariances — the last only when some run has
 * a cluster of its own factor); rvll_live_runs_step makes 1.  RVLL_E_UNSUPPORTED: ndim above 64.
 *
 * rvll_live_runs_clusters  what the last successful clustered step found for its listed run a (0 .. A - 1): *nsurv = m,
 *                          *nclusters, labels [m] of the survivors in rank order, scale [ndim], factors [max(nclusters, 1),
 *                          ndim, ndim] (the walk's factor of every cluster; the global one alone when there is one cluster),
 *                          phase_s [3]: host seconds between the step's synchronisations — clustering and label sort, cluster
 *                          moments, walk.  Any pointer may be NULL.  RVLL_E_INVALID: no clustered step since the live sets
 *                          were loaded, or a out of range.                                                                     */
int rvll_live_runs_step_clustered(rvll_handle* h, const int32_t* runs /*[A]*/, int32_t A, int64_t kdead, const int32_t* ranks /*[A, kdead]*/,
                                  const double* lstar /*[A]*/, const int32_t* wrapped /*[ndim] or NULL*/, int32_t nsteps,
                                  int32_t max_rounds, const uint64_t* seeds /*[A]*/, int32_t nboot, const uint64_t* boot_seeds /*[A]*/,
                                  int64_t* ncalls /*[A] or NULL*/, double* logl_new /*[A, kdead]*/, int32_t* nclusters /*[A]*/);
int rvll_live_runs_clusters(rvll_handle* h, int32_t a, int64_t* nsurv, int32_t* nclusters, int32_t* labels /*[m]*/,
                            double* scale /*[ndim]*/, double* factors /*[max(nclusters, 1), ndim, ndim]*/, double* phase_s /*[3]*/);
/* Birth contours of the resident rows (the insertion-index test; evidence_amd/insertion.py).  A row loaded by
 * rvll_live_init / rvll_live_runs_init is born at -inf; a row a step draws is born at that step's lstar (its run's, for the
 * ensemble steps) — the highest log-L of the batch that died.  The dying rows' births go to the dead store with their theta and
 * log-L, and a step that fails leaves every birth as it was.
 * rvll_live_births       as rvll_live_dead: *n_dead in: capacity of dead_birth [*] (ignored when it is NULL), out: rows in the dead
 *                        store; dead_birth in death order, live_birth [N] (may be NULL) the live rows' as rvll_live_get orders them.
 *                        RVLL_E_INVALID while an ensemble is loaded, or live_birth without a live set.
 * rvll_live_runs_births  the same for run r of the ensemble: dead_birth in the order rvll_live_runs_dead gives, live_birth [n]. */
int rvll_live_births(rvll_handle* h, int64_t* n_dead, double* dead_birth /*[*n_dead] or NULL*/, double* live_birth /*[N] or NULL*/);
int rvll_live_runs_births(rvll_handle* h, int32_t run, int64_t* n_dead, double* dead_birth /*[*n_dead] or NULL*/,
                          double* live_birth /*[n] or NULL*/);

/* ---- scalar-callback latency ------------------------------------------------------------------------- */
/* PolyChord's loglike(theta) is irreducibly scalar (evidence/polychord/__init__.py:166-171): one theta per call.
 * With the server enabled, rvll_loglike_batch(B = 1) is answered by a persistent one-workgroup kernel that polls
 * a block of host-coherent pinned memory: the call writes theta and a request number there and spins on the
 * answer — a PCIe round trip instead of a kernel launch plus a stream synchronisation, same bits.  The kernel
 * leaves by itself after 5 ms without a request and is restarted by the next scalar call; every other entry point
 * of the handle stops it first.  enable = 0 turns it off (default; RVLL_SCALAR_SERVER=1 in the environment turns
 * it on at rvll_create).  While it runs, calls that synchronise the whole device (hipMalloc / hipFree, also of
 * other handles in the process) wait until it is idle, i.e. at most the 5 ms, provided no other thread keeps
 * feeding it meanwhile.  Round 4: up to 64 parameters the request word travels beside every value of the row (keyed with the
 * value, so a torn read cannot pass for a request), the kernel sees request and row in ONE read and answers from its LDS sums:
 * 9.7 - 10.3 us a call on an MI355X (10.8 before), 15.5 us for PolyChord's prior + loglike pair as one request.            */
int rvll_scalar_server(rvll_handle* h, int32_t enable);

/* ---- device-resident forms (no PCIe inside; used by bench and multi-GPU) -- */
/* Reserve device buffers for up to B points and copy theta (or cube) in.     */
int rvll_dev_reserve(rvll_handle* h, int64_t B);
int rvll_dev_upload_theta(rvll_handle* h, const double* theta, int64_t B);
int rvll_dev_upload_cube(rvll_handle* h, const double* cube, int64_t B);
/* Fill the resident cube buffer with counter-based uniforms on the device.   */
int rvll_dev_fill_cube(rvll_handle* h, int64_t B, uint64_t seed);
/* Launch on the handle's compute stream; asynchronous.                        */
int rvll_dev_prior(rvll_handle* h, int64_t B);                 /* cube -> theta  */
int rvll_dev_loglike(rvll_handle* h, int64_t B);               /* theta -> logL  */
/* One launch: the log-L kernel's staging step applies the prior transform to the resident cube rows, keeps
 * theta in LDS for the evaluation and writes it to the resident theta buffer too (prior(cube) followed by
 * loglike(theta) of evidence/polychord/__init__.py:130-171 for a whole batch).  Results are bit-identical to
 * rvll_dev_prior followed by rvll_dev_loglike.                                                           */
int rvll_dev_prior_loglike(rvll_handle* h, int64_t B);         /* cube -> theta, logL */
int rvll_dev_download(rvll_handle* h, int64_t B, double* theta /*or NULL*/,
                      double* logL /*or NULL*/, int32_t* flags /*or NULL*/);
int rvll_dev_sync(rvll_handle* h);
/* Device-resident launches run on one of two pipeline lanes (own stream, log-L and flags buffer each).  Flipping
 * the lane between independent batches keeps two launches in flight, so one batch's ramp-up hides the previous
 * one's tail; rvll_allgather_logl advances it by itself.  Returns the lane the next launch will use.          */
int rvll_dev_flip_lane(rvll_handle* h);
/* Time `iters` log-L launches over the resident theta with HIP events on the
 * compute stream (after `warmup` untimed launches).                          */
int rvll_dev_time_loglike(rvll_handle* h, int64_t B, int32_t warmup, int32_t iters,
                          rvll_timing* out);

/* Two HIP events on the compute stream (lane 0): record which = 0 before and which = 1 after a sequence of
 * device-resident launches; rvll_dev_mark_elapsed waits for the second and returns the time between them as the
 * device saw it (what bench.py divides by its step count for the roofline's kernel duration).               */
int rvll_dev_mark(rvll_handle* h, int32_t which);
int rvll_dev_mark_elapsed(rvll_handle* h, double* ms);

/* ---- launch geometry ------------------------------------------------------ */
/* points_per_block <= 0 restores the built-in heuristic.                     */
int rvll_set_points_per_block(rvll_handle* h, int32_t points_per_block);
/* The log-L kernel has two launch forms with bit-identical results: 256-thread tiles of a few points (small
 * batches, the walk, the scalar calls) and the CU-wide form (one 1024-thread workgroup per CU walking its share of
 * the batch; large batches).  0 = choose by batch size (default), 1 = tiles only, 2 = CU-wide wherever it fits.
 * Environment RVLL_FORM=tile|cu sets the same at rvll_create.                                                  */
int rvll_set_kernel_form(rvll_handle* h, int32_t form);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ----------------------- */
/* 128-byte opaque id created on rank 0 and handed to every rank out of band.  */
#define RVLL_COMM_ID_BYTES 128
int rvll_comm_unique_id(unsigned char id[RVLL_COMM_ID_BYTES]);
int rvll_comm_init(rvll_handle* h, const unsigned char id[RVLL_COMM_ID_BYTES],
                   int32_t nranks, int32_t rank);
/* rvll_comm_init gives ONE pipeline lane (the gather runs in-stream behind its kernel).  Further lanes — a stream,
 * a communicator (ncclCommSplit of the first) and buffers each, so that the gather of step k overlaps the kernel of
 * step k+1 — are added collectively: every rank calls rvll_comm_add_lanes, the ranks agree on the minimum of the
 * counts it returned (out of band), and every rank calls rvll_comm_set_lanes with that number.  Ranks cycling
 * through different numbers of communicators would hang their collectives.                                    */
int rvll_comm_add_lanes(rvll_handle* h, int32_t want, int32_t* have);
int rvll_comm_set_lanes(rvll_handle* h, int32_t nlanes);
/* All-gather of a small host buffer over the same communicator (n_local doubles per rank up, nranks * n_local
 * back, rank-major): what a sampler that shards host-side state over the ranks exchanges per iteration.        */
int rvll_allgather_host(rvll_handle* h, const double* mine, int64_t n_local, double* all /*[nranks * n_local]*/);
/* Which libraries this process actually runs on, as a JSON object: HIP runtime version and path of libamdhip64,
 * path and version of the librccl that was loaded (RVLL_RCCL_PATH, else the one next to that libamdhip64, else
 * /opt/rocm/lib, else by soname), path of librvll itself, and GPU_MAX_HW_QUEUES as the environment has it.
 * ON THAT VARIABLE: the HIP runtime maps a process's streams onto that many hardware queues (default 4) and reads it once, when
 * it starts.  A handle has seven streams; with four queues a copy stream of the streamed host batches
 * (rvll_prior_loglike_batch from 24 MB of rows on) can share the kernels' queue, and a 262144-row call then takes 4.0 ms
 * instead of 2.85 ms with eight (profiles/r04_hw_queues.txt).  Nothing else depends on it (results never do).  librvll
 * never sets the variable: the count is the caller's choice, and "gpu_max_hw_queues_set_by" in the JSON says whether the
 * caller's environment has it.                                                                                         */
int rvll_runtime_info(char* buf, int32_t buflen);
/* One multi-GPU step is rvll_dev_loglike(B_local) followed by rvll_allgather_logl(B_local): every rank's
 * per-shard log-L (the buffer the kernel just wrote) is all-gathered on the device, rank-major, so that every
 * rank — rank 0 owns the sampler's replacement step — holds all nranks*B_local values.  Asynchronous.  Steps
 * alternate between two pipeline lanes (own stream, communicator and buffers each), so the gather of one step
 * overlaps the kernel of the next without cross-stream events; rvll_download_gathered returns the last one. */
int rvll_allgather_logl(rvll_handle* h, int64_t B_local);
int rvll_download_gathered(rvll_handle* h, int64_t B_total, double* logL_all);
/* When theta was produced on the device (rvll_dev_prior / rvll_dev_prior_loglike on a cube shard), the sampler
 * on rank 0 also needs the physical parameters of the points it keeps: one more all-gather, of the B_local x
 * ndim theta rows, rank-major like the log-L gather.  Asynchronous on the compute stream.                    */
int rvll_allgather_theta(rvll_handle* h, int64_t B_local);
int rvll_download_gathered_theta(rvll_handle* h, int64_t B_total, double* theta_all /*[B_total, ndim]*/);
int rvll_comm_destroy(rvll_handle* h);

/* ---- Keplerian curves at arbitrary times (post-processing helper) ------------------ */
/* Replaces RVModel.kep_rv(pardict, time, exclude_planet) and RVModel.modelk(pardict, time, planet)
 * (evidence/rvmodel/__init__.py:343-385, 388-463) as evidence/post_processing.py:413-428 calls them for
 * phase folds: out[b][j] = sum over planets ip with bit ip of include_mask set of the Keplerian RV of
 * theta[b] at times[j].  kep_rv(exclude_planet=k) is mask = all bits but k-1; modelk(planet=k) is
 * mask = 1 << (k-1).  An invalid orbit (the reference returns None) gives a NaN row.                  */
int rvll_kep_rv_batch(rvll_handle* h, const double* theta, int64_t B, const double* times,
                      int32_t n_times, uint32_t include_mask, double* out /*[B, n_times]*/);

/* Order statistics of groups of those curves (evidence_amd/predictive.py is the definition).  theta holds n_groups
 * groups of n rows; the curves of every row are rvll_kep_rv_batch's, bit for bit (the same kernel writes them into a device
 * buffer).  Per group g and time j, over the n curve values of the group at that time: n_valid[g][j] = how many are not NaN;
 * with those sorted ascending, q[g][k][j] = sorted[max(0, ceil(levels[k] * n_valid) - 1)] (the product in double: the inverted
 * CDF of equal weights) and mean[g][j] = their sum taken from left to right in sorted order, over n_valid; NaN where n_valid
 * is 0.  The work goes in chunks of whole groups whose curve values take at most chunk_bytes (0: 256 MiB; at least one group);
 * the results do not depend on it.  phase_ms (may be NULL) receives the HIP-event time of the curve kernel and of the sort.
 * RVLL_E_INVALID: n outside [1, 4096], n_q outside [1, 16], a level outside (0, 1), a negative size, null buffers.          */
int rvll_kep_rv_bands(rvll_handle* h, const double* theta /*[n_groups * n, ndim]*/, int64_t n_groups, int32_t n,
                      const double* times, int32_t n_times, uint32_t include_mask, const double* levels /*[n_q]*/, int32_t n_q,
                      double* q /*[n_groups, n_q, n_times]*/, double* mean /*[n_groups, n_times]*/,
                      int32_t* n_valid /*[n_groups, n_times]*/, int64_t chunk_bytes, double* phase_ms /*NULL or [2]*/);

/* ---- residuals of the likelihood's model and their periodograms (post-processing; evidence_amd/periodogram.py) ---- */
/* res[b][j] and var[b][j] are `res` and `noise` of RVModel.log_likelihood (evidence/rvmodel/__init__.py:180-215) for theta[b] at
 * epoch j of the resident table: the datum minus the instrument's offset, the Keplerian sum of the planets in include_mask
 * (rvll_kep_rv_batch's value at the table's times, bit for bit), the drift about drift_tref or the table's first time, and the
 * linear terms, added in that order; var = svrad^2 (+ jitter^2 of the instrument).  An invalid orbit gives a NaN row of res.
 * Nothing is uploaded except theta.                                                                                        */
int rvll_residuals_batch(rvll_handle* h, const double* theta, int64_t B, uint32_t include_mask, double* res /*[B, Ne]*/,
                         double* var /*[B, Ne]*/);

/* Generalised Lomb-Scargle powers (floating mean, Zechmeister & Kuerster 2009) of those residuals on the uniform grid
 * f_k = f0 + df k, k < n_freq, with weights 1 / var, and per group of n rows what rvll_kep_rv_bands gives with the frequencies in
 * the place of times: q, mean, n_valid.  peak_index[g][i] is the first index of row i's largest power (a NaN power counts as the
 * largest) and peak_power the power there; -1 and NaN for a row whose powers are all NaN (an invalid orbit).  power_out (may be NULL) receives every
 * power.  A power is NaN where YY D is not > 0.  The work goes in chunks of whole groups whose powers and weights take at most
 * chunk_bytes (0: 256 MiB; at least one group); no result depends on it, nor on the other rows or groups of the call.  phase_ms
 * (may be NULL) receives the HIP-event times of the residual stage, the periodogram kernel and the reductions.
 * RVLL_E_INVALID: f0 or df not positive and finite, n_freq outside [1, 2^24], fewer than 4 epochs, n outside [1, 4096], n_q
 * outside [1, 16], a level outside (0, 1), a negative size, null buffers.                                                   */
int rvll_gls_bands(rvll_handle* h, const double* theta /*[n_groups * n, ndim]*/, int64_t n_groups, int32_t n, uint32_t include_mask,
                   double f0, double df, int32_t n_freq, const double* levels /*[n_q]*/, int32_t n_q,
                   double* q /*[n_groups, n_q, n_freq]*/, double* mean /*[n_groups, n_freq]*/, int32_t* n_valid /*[n_groups, n_freq]*/,
                   int32_t* peak_index /*[n_groups, n]*/, double* peak_power /*[n_groups, n]*/,
                   double* power_out /*NULL or [n_groups, n, n_freq]*/, int64_t chunk_bytes, double* phase_ms /*NULL or [3]*/);

/* ---- log-likelihood under correlated noise: celerite kernels (evidence_amd/correlated.py) ---- */
/* The covariance of the residuals above is diag(var) + K, K[n][m] = sum over the terms of k(|t_n - t_m|) (Foreman-Mackey et
 * al. 2017).  A term's parameters par[] are slots like every other model scalar: theta[idx], or the constant val when idx < 0.
 *   RVLL_NOISE_REAL      par = sigma, tau                 k = sigma^2 exp(-x / tau)                              1 column
 *   RVLL_NOISE_SHO       par = sigma, rho, q              celerite2's SHOTerm: w0 = 2 pi / rho, S0 = sigma^2 / (w0 q)   2 columns
 *   RVLL_NOISE_ROTATION  par = sigma, prot, q0, dq, mix   celerite2's RotationTerm: two SHOs at prot and prot / 2       4 columns
 * |q - 1/2| of an SHO is taken as at least 1e-6 on the side q lies on (q = 1/2 counts as above).  At most
 * RVLL_NOISE_MAX_TERMS terms and RVLL_NOISE_MAX_RANK columns in all.                                                        */
#define RVLL_NOISE_REAL 0
#define RVLL_NOISE_SHO 1
#define RVLL_NOISE_ROTATION 2
#define RVLL_NOISE_MAX_TERMS 4
#define RVLL_NOISE_MAX_RANK 4
#define RVLL_FLAG_NOISE_INVALID 8   /* the noise parameters of this row give no positive definite covariance -> logL=-1e30 */
typedef struct rvll_noise_term { int32_t kind; int32_t reserved; rvll_slot par[5]; } rvll_noise_term;

/* logl[b] = -1/2 r^T (diag(var) + K)^-1 r - 1/2 ln det(diag(var) + K) - Ne/2 ln(2 pi) with r, var = rvll_residuals_batch's of row
 * b with every planet subtracted, by the O(Ne J^2) factorisation of the semiseparable covariance (csrc/rvll_celerite.h), one row
 * a lane.  x holds theta rows, or with from_cube = 1 unit-cube rows that go through rvll_dev_upload_cube + rvll_dev_prior first
 * (theta_out, if not NULL, receives rvll_prior_batch's theta, bit for bit).  order lists the epochs in nondecreasing time (ties
 * in any order; NULL: the table is in that order already).  flags: RVLL_FLAG_INVALID_ORBIT alone for an invalid orbit (logl
 * -1e30); RVLL_FLAG_NOISE_INVALID (logl -1e30) for noise parameters that are not finite, sigma < 0, mix < 0, tau, rho, q, prot,
 * q0 + 1/2 or dq not > 0, or a pivot of the factorisation that is not > 0.  The rows go in chunks whose residuals and variances
 * take at most 256 MiB; a row's bits depend on that row and the epoch table alone.  phase_ms (may be NULL) receives the
 * HIP-event times of the residual stage and of the solve.
 * RVLL_E_INVALID: an order that is not a permutation or whose times decrease, n_terms outside [1, RVLL_NOISE_MAX_TERMS], more
 * than RVLL_NOISE_MAX_RANK columns, an unknown kind, a slot index >= ndim, null buffers, a negative B.  RVLL_E_UNSUPPORTED: a
 * handle whose precision is not RVLL_PREC_FP64.  RVLL_E_NOPRIORS: from_cube without rvll_set_priors.                        */
int rvll_celerite_loglike_batch(rvll_handle* h, const double* x /*[B, ndim]: theta, or unit cubes*/, int64_t B,
                                int32_t from_cube, const rvll_noise_term* terms, int32_t n_terms,
                                const int32_t* order /*[Ne] epochs in nondecreasing time, NULL: table order*/,
                                double* theta_out /*NULL, or [B, ndim] when from_cube*/, double* logl /*[B]*/,
                                int32_t* flags /*[B]*/, double* phase_ms /*NULL or [2]: residual stage, solve*/);

/* The GP those terms define, given the data (evidence_amd/correlated.py: predict_dense): with r, var and
 * Sigma = diag(var) + K as above and alpha = Sigma^-1 r,
 *   residual[b][n]   r, the datum minus the full deterministic model
 *   mean_data[b][n]  the mean of the latent GP at epoch n given all data, r_n - var_n alpha_n
 *   var_data[b][n]   its variance, var_n - var_n^2 (Sigma^-1)_nn
 *   mean[b][i]       sum over n of k(|times[i] - t_n|) alpha_n, the mean at a query time
 *   var[b][i]        k(0) - K(x, t) Sigma^-1 K(t, x) at x = times[i]; only with want_var, O(M Ne J) a row where everything else
 *                    is O((Ne + M) J^2)
 * [B, Ne] in the order of the epoch table, [B, M] in the order of times, which need not be sorted; every time enters as its
 * float64 difference from the first epoch in time order.  logl and flags are rvll_celerite_loglike_batch's, bit for bit; a row
 * with a flag has NaN in every array.  The rows go in chunks whose device buffers take at most 256 MiB (at least 64 rows); a
 * row's bits depend on that row, the epoch table and the query times alone.  phase_ms (may be NULL) receives the HIP-event
 * times of the residual stage, the factor sweep, the backward and forward sweeps, and the variance at the query times.
 * RVLL_E_INVALID: what rvll_celerite_loglike_batch refuses, a negative M, a time that is not finite, var without want_var, null
 * buffers.  RVLL_E_UNSUPPORTED: a handle whose precision is not RVLL_PREC_FP64.                                              */
int rvll_celerite_predict_batch(rvll_handle* h, const double* theta /*[B, ndim]*/, int64_t B, const rvll_noise_term* terms,
                                int32_t n_terms, const int32_t* order /*[Ne] epochs in nondecreasing time, NULL: table order*/,
                                const double* times /*[M], NULL when M = 0*/, int64_t M, int32_t want_var,
                                double* residual /*[B, Ne] or NULL*/, double* mean_data /*[B, Ne]*/, double* var_data /*[B, Ne] or NULL*/,
                                double* mean /*[B, M], NULL when M = 0*/, double* var /*[B, M] with want_var, else NULL*/,
                                double* logl /*[B]*/, int32_t* flags /*[B]*/,
                                double* phase_ms /*NULL or [4]: residuals, factor, sweeps, grid variance*/);

/* ---- FIP periodogram accumulation (post-processing; independent of any model handle) ------------ */
/* Replaces the accumulation loop of evidence/fip_criterion.py:305-339.  The caller flattens the posterior
 * samples of all planet models of one run into rows, in the reference's loop order (kmod = 1.., then sample
 * i), NaN-padding each row to np_max periods, with contrib[row] = pky[kmod] * weights[i] / sum(weights)
 * (:315, :339); rows of run r are run_start[r] .. run_start[r+1].  nua/nub are the window edges
 * nu -/+ nu_window/2 of :233-236 (ascending).  For every row and period x:  f = 2*pi/x,
 * beg = searchsorted(nub, f, 'right'), end = searchsorted(nua, f, 'left'); every bin in the UNION of the
 * row's [beg, end) ranges gets fapnu[r][bin] -= contrib[row], in row order (numpy's fancy-index `-=` applies
 * a repeated index once).  fapnu is [n_runs, nfreq], in/out (the reference starts from ones, :307); the
 * result is bit-identical to the reference's loop.  `repeats` > 1 re-runs the two kernels from the same
 * input for timing; timing may be NULL.  device < 0 uses the current device.                            */
#define RVLL_FIP_MAX_PLANETS 8
typedef struct rvll_fip_timing {
    double  index_ms;        /* mean HIP-event time of the interval (searchsorted) kernel   */
    double  accumulate_ms;   /* mean HIP-event time of the ordered fold kernel              */
    int64_t rows;
    int32_t repeats;
    int32_t reserved;
} rvll_fip_timing;
int rvll_fip_accumulate(int32_t device, const double* nua, const double* nub, int32_t nfreq,
                        const double* periods /*[rows, np_max]*/, const double* contrib /*[rows]*/,
                        const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs, int32_t np_max,
                        double* fapnu /*[n_runs, nfreq] in/out*/, int32_t repeats, rvll_fip_timing* timing);

/* ---- simulated shrinkage of finished runs (post-processing; independent of any model handle) ---------- */
/* Replicates of ln Z, the information H and the posterior weights of R finished nested-sampling runs, each death's prior
 * shrinkage redrawn (Skilling 2006; Higson et al. 2018).  evidence_amd/shrinkage.py is the definition.
 * Rows run_start[r] .. run_start[r+1] of logl (n_rows in all) are run r: n_dead[r] dead points in death order, then its
 * m = rows - n_dead[r] >= 1 final live points.  Death j of run r dies with n_j = nlive[r] - (j mod kbatch[r]) live points and
 * shrinks the prior volume by log t_j = log(1 - uniform01(seed, j)) / n_j, seed = seeds[r] + s * 0xD1B54A32D192ED03 for
 * replicate s (RVLL_SHRINK_EXPECTED: log t_j = -1 / n_j).  logX_j = logX_{j-1} + log t_j from 0; a dead row weighs
 * logl_j + logX_{j-1} + log(-expm1(log t_j)), a live row logX_last - log(m) + logl_i.  Out: logz[r * nsamples + s] =
 * logsumexp of every row, info[r * nsamples + s] = the dead rows' information (sum w logl / Zd - ln Zd; 0 without weight),
 * and, if logwt is not NULL, logwt[nsamples * run_start[r] + s * rows + i] = weight - ln Z (the caller's buffer of
 * nsamples * n_rows doubles).  The weights go through a device block of at most block_bytes (0: 512 MiB), some replicates of
 * every run at a time; RVLL_E_NOMEM, before any work, when one replicate of all runs does not fit.  RVLL_E_INVALID for a
 * run_start that does not rise from 0 to n_rows, n_dead < 0, kbatch < 1, kbatch >= nlive, n_dead % kbatch != 0, m < 1,
 * nsamples < 1 and negative sizes.  A (run, replicate)'s results do not depend on the other runs of the call.  timing may be
 * NULL.  device < 0 uses the current device.                                                                         */
#define RVLL_SHRINK_RANDOM 0
#define RVLL_SHRINK_EXPECTED 1
typedef struct rvll_shrink_timing {
    double  kernel_ms;       /* HIP-event time of the replicate kernels, summed over the launches */
    double  total_ms;        /* the whole call: allocation, uploads, kernels, downloads           */
    int64_t elements;        /* (row, replicate) pairs: n_rows * nsamples                          */
    int32_t launches;
    int32_t threads;         /* per workgroup; one workgroup per (run, replicate)                  */
} rvll_shrink_timing;
int rvll_shrinkage_replicates(int32_t device, const double* logl, int64_t n_rows, const int64_t* run_start /*[n_runs + 1]*/,
                              int32_t n_runs, const int64_t* n_dead, const int32_t* nlive, const int32_t* kbatch,
                              const uint64_t* seeds, int32_t nsamples, int32_t mode, double* logz /*[n_runs, nsamples]*/,
                              double* info /*[n_runs, nsamples]*/, double* logwt /*NULL or [nsamples * n_rows]*/,
                              int64_t block_bytes, rvll_shrink_timing* timing);

/* ---- insertion indexes of finished runs (post-processing; independent of any model handle) ---------------- */
/* The insertion-index test (Fowlie, Handley & Su 2020): evidence_amd/insertion.py is the definition.  Rows
 * run_start[r] .. run_start[r+1] of logl / birth (n_rows in all, any order inside a run) are run r.  For a row j with
 * birth b = birth[j] > -inf: live(j) = {k in its run : birth[k] <= b < logl[k]}, n_at_out[j] = |live(j)|, index_out[j] =
 * #{k in live(j) : logl[k] < logl[j]}; rows with birth -inf get -1 in both.  Doubles are compared as doubles (-0.0 == +0.0).
 * The outputs are integers: the same for a run alone or inside any batch.  RVLL_E_INVALID for NaN values, a run_start that
 * does not rise from 0 to n_rows, n_runs < 1, runs of 2^31 rows or more, and null buffers.  timing may be NULL.  device < 0
 * uses the current device.                                                                                               */
typedef struct rvll_insertion_timing {
    double  kernel_ms;       /* HIP-event time of the device work (key map, two segmented sorts, counts), summed over chunks */
    double  total_ms;        /* the whole call: checks, allocation, uploads, kernels, downloads                            */
    int64_t rows;            /* n_rows                                                                                      */
    int32_t launches;        /* kernel launches issued (a rocPRIM sort counted as one)                                      */
    int32_t threads;         /* per workgroup; one wave64 per row                                                           */
} rvll_insertion_timing;
int rvll_insertion_indexes(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                           const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs, int32_t* index_out /*[n_rows]*/,
                           int32_t* n_at_out /*[n_rows]*/, rvll_insertion_timing* timing);

/* ---- merging finished runs by their birth contours (post-processing; independent of any model handle) ------------ */
/* R runs become one run whose live count varies from death to death (Higson et al. 2018; dynesty's merge_runs).
 * evidence_amd/merge.py is the definition.  Rows run_start[r] .. run_start[r+1] of logl / birth (n_rows in all,
 * any order inside a run) are run r.  The merged order sorts every row stably by log-L, ties by run and then by position, so
 * order_out[i] is the input row (run_start[r] + position) of merged row i.  A row with logl <= birth counts with the birth
 * nextafter(logl, -inf) (*n_off_contour of them).  With run multiplicities w_r (1 each without the bootstrap), merged row i
 * dies at n_i = sum_{birth_k < logl_i} w - sum_{k < i} w live points, w_{rho_i} times in a row at n_i, n_i - 1, ...; its
 * shrinkage Delta_i sums -1 / (n_i - q) (RVLL_SHRINK_EXPECTED) or log(1 - uniform01(seed_s, c)) / (n_i - q) over q < w, c the
 * copies that died before, seed_s = seed + s * 0xD1B54A32D192ED03.  logw_i = (logl_i + logX_{i-1}) + log(-expm1(Delta_i)),
 * logz = logsumexp(logw), info = sum e^{logw - logz} logl - logz, logwt = logw - logz.  Bootstrap: w_r counts r among the
 * draws floor(uniform01(seed_s ^ 0x5851F42D4C957F2D, t) * n_runs), t < n_runs.
 * rvll_merge_runs: the merged run itself (expected shrinkage, no bootstrap): order_out, nlive_out (n_i), logz, info and
 * logwt_out [n_rows] in merged order.  rvll_merge_replicates: logz[s], info[s] of nsamples replicates and, if logwt is not
 * NULL, logwt[s * n_rows + i]; the weights go through a device block of at most block_bytes (0: 512 MiB), RVLL_E_NOMEM before
 * any work when one replicate does not fit.  A replicate's results do not depend on the others of the call.
 * RVLL_E_INVALID: n_runs < 1, n_rows outside [1, 2^30), a run_start that does not rise from 0 to n_rows, NaN births, NaN or
 * infinite log-L, nsamples < 1, an unknown mode, bootstrap not 0 / 1, bootstrap with more than 8192 runs, negative
 * block_bytes, null buffers.  timing may be NULL.  device < 0 uses the current device.                                     */
typedef struct rvll_merge_timing {
    double  kernel_ms;       /* HIP-event time of the device work (keys, two radix sorts, placement, replicate kernels)  */
    double  total_ms;        /* the whole call: checks, allocation, uploads, kernels, downloads                          */
    int64_t rows;            /* n_rows                                                                                    */
    int64_t elements;        /* (row, replicate) pairs: n_rows * nsamples (n_rows for rvll_merge_runs)                    */
    int32_t launches;        /* kernel launches issued (a rocPRIM sort counted as one)                                    */
    int32_t threads;         /* per workgroup of the replicate kernel; one workgroup per replicate                       */
} rvll_merge_timing;
int rvll_merge_runs(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                    const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs, int64_t* order_out /*[n_rows]*/,
                    int64_t* nlive_out /*[n_rows]*/, double* logz, double* info, double* logwt_out /*[n_rows]*/,
                    int64_t* n_off_contour, rvll_merge_timing* timing);
int rvll_merge_replicates(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                          const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs, int32_t nsamples, int32_t mode,
                          int32_t bootstrap, uint64_t seed, double* logz /*[nsamples]*/, double* info /*[nsamples]*/,
                          double* logwt /*NULL or [nsamples * n_rows]*/, int64_t block_bytes, rvll_merge_timing* timing);

/* ---- posterior summaries of the merged run's replicates (post-processing; independent of any model handle) ------- */
/* Per replicate s of rvll_merge_replicates (same seeds, multiplicities and merged order) and per column c of values
 * [n_rows, n_cols] (row-major, in input row order; any parameter or derived quantity), with p_i = exp(logwt_i) (0 for a row
 * without weight), P = sum p and x_i the column's value in merged row i (evidence_amd/posterior.py is the definition, DESIGN
 * §4k):  mean[s * n_cols + c] = sum p x / P;  sd[s * n_cols + c] = sqrt(sum p (x - mean)^2 / P), the spread about the
 * replicate's own mean;  quant[(s * n_q + k) * n_cols + c] = the inverted weighted CDF at quantiles[k]: x of the first row, in
 * the order of x, whose inclusive running sum of p reaches quantiles[k] * P (numpy's quantile(x, q, weights=p,
 * method="inverted_cdf")); and logz[s], info[s] as rvll_merge_replicates gives them.  The weights stay on the device: a block
 * of replicates is reduced where it was written.  block_bytes bounds the per-call tables (values in merged order and one
 * permutation a column: 12 * n_rows * n_cols bytes) plus the block of weights (8 * n_rows a replicate); 0 stands for the
 * tables plus 8 GiB, of which only nsamples replicates are allocated.  RVLL_E_NOMEM before any work when the tables and one
 * replicate do not fit.  A replicate's results do not depend on the others of the call or on the batching.  A replicate in
 * which no row has weight (a bootstrap of empty runs) gives NaN.
 * RVLL_E_INVALID: everything rvll_merge_replicates refuses; n_cols outside [1, 64], n_q outside [1, 16], a level outside the
 * open interval (0, 1), a value that is not finite, null buffers.  timing may be NULL.  device < 0 uses the current device. */
typedef struct rvll_posterior_timing {
    double  kernel_ms;       /* HIP-event time of all device work: setup_ms + weights_ms + reduce_ms                       */
    double  total_ms;        /* the whole call: checks, allocation, uploads, kernels, downloads                            */
    double  setup_ms;        /* the merge's setup, the permutation of values and one radix sort a column                    */
    double  weights_ms;      /* the replicate kernels (what rvll_merge_replicates spends on the same input)                 */
    double  reduce_ms;       /* exp of the block and the (replicate, column) summary kernel                                 */
    int64_t rows;            /* n_rows                                                                                      */
    int64_t elements;        /* (row, replicate) pairs: n_rows * nsamples                                                   */
    int32_t launches;        /* 5 + 2 * n_cols for the setup, then 3 a block of replicates (a rocPRIM sort counted as one)  */
    int32_t threads;         /* per workgroup; one workgroup per replicate (weights) and per (replicate, column) (summary)  */
    int32_t blocks;          /* blocks of replicates the call was split into                                                */
    int32_t reserved;
} rvll_posterior_timing;
int rvll_posterior_replicates(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                              const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs,
                              const double* values /*[n_rows * n_cols]*/, int32_t n_cols, const double* quantiles /*[n_q]*/,
                              int32_t n_q, int32_t nsamples, int32_t mode, int32_t bootstrap, uint64_t seed,
                              double* logz /*[nsamples]*/, double* info /*[nsamples]*/, double* mean /*[nsamples * n_cols]*/,
                              double* sd /*[nsamples * n_cols]*/, double* quant /*[nsamples * n_q * n_cols]*/,
                              int64_t block_bytes, rvll_posterior_timing* timing);

/* ---- pointwise predictive checks of the merged run's replicates (post-processing; independent of any model handle) */
/* Per replicate s of rvll_merge_replicates (same seeds, multiplicities and merged order) and per unit u of table [n_rows,
 * n_units] (row-major, in input row order: the log-likelihood of the unit's data in the row), with p_i = exp(logwt_i) (0 for a
 * row without weight), P = sum p, t the unit's value in merged row i and the call's shifts [3, n_units] = (c, d, a)
 * (evidence_amd/pointwise.py is the definition and computes the shifts):
 *     lpd [s * n_units + u] = c_u + log(sum p exp(min(t - c_u, 0)) / P)     the in-sample log predictive density
 *     loo [s * n_units + u] = d_u - log(sum p exp(min(d_u - t, 0)) / P)     the importance-sampling leave-one-out value
 *     mean[s * n_units + u] = a_u + sum p (t - a_u) / P
 *     var [s * n_units + u] = sum p (t - a_u)^2 / P - (sum p (t - a_u) / P)^2     the WAIC correction
 * and logz[s], info[s] as rvll_merge_replicates gives them.  With c_u >= t and d_u <= t on every row with weight the two min
 * change nothing; they keep exp finite on the others.  The sums are one fp64 product on the matrix units, [replicates, n_rows]
 * by [n_rows, 4 n_units + 1], cut along n_rows into slabs of rvll_pointwise_slab_rows rows (a constant) that are added in
 * rising order: a result depends on the input, the seed and the replicate's index, not on the batching, on the other units of
 * the call or on the call.  P is a column of that product, so a unit whose t is one constant v (and c = d = a = v) gives lpd =
 * loo = mean = v exactly and var = 0.  A replicate in which no row has weight gives NaN.
 * block_bytes bounds the operand (8 bytes * (n_rows rounded up to 64) * (4 n_units + 1 rounded up to 64)), the partial sums
 * of 64 replicates (8 * 64 * slabs * columns) and the block of replicates (8 * (n_rows + slabs * columns) each); 0 stands for
 * the first two plus 8 GiB.  RVLL_E_NOMEM before any work when these and one replicate do not fit.
 * RVLL_E_INVALID: everything rvll_merge_replicates refuses; n_units outside [1, 4096]; a table value or a shift that is not
 * finite or is beyond 1e30 in size; null buffers.  timing may be NULL.  device < 0 uses the current device. */
typedef struct rvll_pointwise_timing {
    double  kernel_ms;       /* HIP-event time of all device work: setup_ms + weights_ms + reduce_ms                       */
    double  total_ms;        /* the whole call: checks, allocation, uploads, kernels, downloads                            */
    double  setup_ms;        /* the merge's setup and the kernel that writes the operand                                    */
    double  weights_ms;      /* the replicate kernels (what rvll_merge_replicates spends on the same input)                 */
    double  reduce_ms;       /* exp of the block, the product and the kernel that adds the slabs                            */
    int64_t rows;            /* n_rows                                                                                      */
    int64_t elements;        /* (row, replicate) pairs: n_rows * nsamples                                                   */
    int64_t columns;         /* 4 * n_units + 1: the product takes 2 * elements * columns operations                        */
    int32_t launches;        /* 5 for the setup, then 4 a block of replicates (a rocPRIM sort counted as one)               */
    int32_t threads;         /* per workgroup                                                                               */
    int32_t blocks;          /* blocks of replicates the call was split into                                                */
    int32_t slabs;           /* slabs of rows: n_rows over rvll_pointwise_slab_rows, rounded up                             */
} rvll_pointwise_timing;
int rvll_pointwise_replicates(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                              const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs,
                              const double* table /*[n_rows * n_units]*/, int32_t n_units, const double* shifts /*[3 * n_units]*/,
                              int32_t nsamples, int32_t mode, int32_t bootstrap, uint64_t seed,
                              double* logz /*[nsamples]*/, double* info /*[nsamples]*/, double* lpd /*[nsamples * n_units]*/,
                              double* loo /*[nsamples * n_units]*/, double* mean /*[nsamples * n_units]*/,
                              double* var /*[nsamples * n_units]*/, int64_t block_bytes, rvll_pointwise_timing* timing);
int rvll_pointwise_slab_rows(int32_t* rows);

/* ---- prior densities (post-processing; independent of any model handle) ------------------------------------------- */
/* The log density of the transform rvll_prior_batch applies, per kind (csrc/rvll_prior_density.h; evidence_amd/priors.py,
 * log_density, is the numpy definition): -inf outside the support, NaN for a NaN argument.  A descriptor is apart
 * from rvll_prior, whose table kinds do not carry their shape parameters.  Arguments and supports:
 *     SKIP               -                                    contributes 0 whatever theta is
 *     UNIFORM            xmin, xmax                           [xmin, xmax]
 *     JEFFREYS           xmin, xmax                           [xmin, xmax]
 *     MODJEFFREYS        x0, xmax                             [0, xmax]
 *     UNIFORMFREQUENCY   xmin, xmax                           [xmin, xmax]
 *     NORMAL             loc, scale                           real line
 *     LOGNORMAL          s, loc, scale                        x > loc
 *     LOG10NORMAL        mu, sigma                            x > 0
 *     TRUNCRAYLEIGH      sigma, xmax                          [0, xmax)
 *     TRUNCUNORMAL       mu, sigma, xmin, xmax, ln dPhi       [xmin, xmax);  dPhi = Phi((xmax-mu)/sigma) - Phi((xmin-mu)/sigma)
 *     POWERLAW           alpha, xmin, xmax, ln A              [xmin, xmax);  A = (1+alpha) / (xmax^(1+alpha) - xmin^(1+alpha))
 *     DOUBLEPOWERLAW     alpha, beta, x0, xmin, xmax, ln A    [xmin, xmax);  A as priors.py:295-297
 *     SINE               lo, hi, ln A                         [lo, hi] = [max(xmin, 0), min(xmax, 180)];  A as priors.py:336
 *     BINORMAL           mu1, sigma1, mu2, sigma2, A          real line
 *     ASYMNORMAL         mu, sigma1, sigma2                   real line
 *     ALPHA              a, Phi(a)                            x > 0
 *     BETA               a, b, ln B(a, b)                     (0, 1)
 *     GAMMA              alpha, beta, ln Gamma(alpha)         x > 0
 *     SORTED_UNIFORM     a, b                                 a <= x_1 <= ... <= x_n <= b over the members of the group
 *     SORTED_LOGUNIFORM  a, b                                 the same; 0 < a
 * The members of a sorted group are the descriptors of one set with the same `group` (>= 0; they must be of one kind), in
 * rising parameter order; the bounds are those of the last member and the joint density, ln n! - n ln(b - a) or ln n! - n ln
 * ln(b / a) - sum ln x_i, is credited once, -inf when the order is broken.                                              */
enum {
    RVLL_DENSITY_SKIP = 0,
    RVLL_DENSITY_UNIFORM = 1,
    RVLL_DENSITY_JEFFREYS = 2,
    RVLL_DENSITY_MODJEFFREYS = 3,
    RVLL_DENSITY_UNIFORMFREQUENCY = 4,
    RVLL_DENSITY_NORMAL = 5,
    RVLL_DENSITY_LOGNORMAL = 6,
    RVLL_DENSITY_LOG10NORMAL = 7,
    RVLL_DENSITY_TRUNCRAYLEIGH = 8,
    RVLL_DENSITY_TRUNCUNORMAL = 9,
    RVLL_DENSITY_POWERLAW = 10,
    RVLL_DENSITY_DOUBLEPOWERLAW = 11,
    RVLL_DENSITY_SINE = 12,
    RVLL_DENSITY_BINORMAL = 13,
    RVLL_DENSITY_ASYMNORMAL = 14,
    RVLL_DENSITY_ALPHA = 15,
    RVLL_DENSITY_BETA = 16,
    RVLL_DENSITY_GAMMA = 17,
    RVLL_DENSITY_SORTED_UNIFORM = 18,
    RVLL_DENSITY_SORTED_LOGUNIFORM = 19,
    RVLL_DENSITY__COUNT
};
#define RVLL_DENSITY_NARGS 8
typedef struct rvll_prior_density {
    int32_t kind;              /* RVLL_DENSITY_*                                                                              */
    int32_t group;             /* sorted kinds: the group's id (>= 0); ignored by the others                                 */
    double  args[RVLL_DENSITY_NARGS];
} rvll_prior_density;
typedef struct rvll_density_timing {
    double  kernel_ms;       /* HIP events around the kernels                                                               */
    double  total_ms;        /* the whole call: checks, allocations, copies, kernels                                        */
    int64_t rows;            /* B                                                                                           */
    int64_t elements;        /* densities evaluated: B * n_sets * ndim                                                      */
    int32_t launches;        /* one a chunk of rows                                                                         */
    int32_t threads;         /* per workgroup                                                                               */
} rvll_density_timing;
/* out[b * n_sets + a] = the sum over d of the log density of sets[a * ndim + d] at theta[b * ndim + d], added in rising d.  A
 * value depends on its row and its set alone: the same bits in any batching.  Stateless; a negative device is the current
 * one.  RVLL_E_INVALID for null buffers, B outside [1, 2^30), ndim outside [1, 64], n_sets outside [1, 4096], an unknown
 * kind, arguments the factories of evidence_amd/priors.py refuse, and a sorted group of mixed kinds.  The rows go to the
 * device in chunks whose theta and out stay within 256 MiB.                                                                */
int rvll_prior_logpdf_batch(int32_t device, const rvll_prior_density* sets /*[n_sets * ndim]*/, int32_t n_sets, int32_t ndim,
                            const double* theta /*[B * ndim]*/, int64_t B, double* out /*[B * n_sets]*/,
                            rvll_density_timing* timing);

/* ---- FIP periodogram of the merged run's replicates (post-processing; independent of any model handle) ----------- */
/* Per replicate s of rvll_merge_replicates (same seeds, multiplicities and merged order) the true inclusion probability of
 * every frequency bin of one planet model (evidence_amd/fip.py, merged_tip_arrays, is the definition).  periods
 * [n_rows, n_planets] is row-major in input row order, finite and positive.  Row i and planet j span the bins [beg, end) with
 * omega = 6.283185307179586 / P_ij, beg = #{nub <= omega}, end = #{nua < omega} (rvll_fip_accumulate's spans; empty when
 * beg >= end); the row covers the union of its spans, a bin once.  With p_i = exp(logwt_i) (0 for a row without weight) and
 * P = sum p:  tip[s * nfreq + b] = sum of p_i over the rows that cover b, over P, clamped to [0, 1]; exactly 0 for a bin that no
 * row covers (decided from integer counts); NaN in a replicate in which no row has weight.  logz[s], info[s] as
 * rvll_merge_replicates gives them.  The weights stay on the device: a block of replicates is reduced where it was written.
 * block_bytes bounds the per-call event tables (with m = n_rows * n_planets and t = ceil(m / 1024): 8 m + 8 nfreq + 8 (t + 1)
 * bytes) plus, a replicate, its weights and its two running sums (8 n_rows + 16 nfreq bytes); 0 stands for the tables plus
 * 8 GiB, of which only nsamples replicates are allocated.  RVLL_E_NOMEM before any work when the tables and one replicate do
 * not fit.  A replicate's results do not depend on the others of the call or on the batching.
 * RVLL_E_INVALID: everything rvll_merge_replicates refuses; n_planets outside [1, RVLL_FIP_MAX_PLANETS], nfreq outside
 * [1, 2^30], n_rows * n_planets >= 2^31, nua or nub that decrease or hold NaN, a period that is not finite and positive, null
 * buffers.  timing may be NULL.  device < 0 uses the current device. */
typedef struct rvll_fip_merged_timing {
    double  kernel_ms;       /* HIP-event time of all device work: setup_ms + weights_ms + reduce_ms                       */
    double  total_ms;        /* the whole call: checks, allocation, uploads, kernels, downloads                            */
    double  setup_ms;        /* the merge's setup, the span kernel, two radix sorts, the count and tile tables              */
    double  weights_ms;      /* the replicate kernels (what rvll_merge_replicates spends on the same input)                 */
    double  reduce_ms;       /* exp and P of the block, the (replicate, list) coverage kernel and the TIP kernel            */
    int64_t rows;            /* n_rows                                                                                      */
    int64_t elements;        /* (row, replicate) pairs: n_rows * nsamples                                                   */
    int64_t events;          /* entries of the two event lists together: 2 * n_rows * n_planets                             */
    int32_t launches;        /* 11 for the setup, then 4 a block of replicates (a rocPRIM sort counted as one)              */
    int32_t threads;         /* per workgroup; one workgroup per replicate (weights, exp) and per (replicate, list)         */
    int32_t blocks;          /* blocks of replicates the call was split into                                                */
    int32_t key_bits;        /* bits of a bin key that the radix sorts pass over: ceil(log2(nfreq + 1))                     */
} rvll_fip_merged_timing;
int rvll_fip_replicates(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                        const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs,
                        const double* periods /*[n_rows * n_planets]*/, int32_t n_planets, const double* nua /*[nfreq]*/,
                        const double* nub /*[nfreq]*/, int32_t nfreq, int32_t nsamples, int32_t mode, int32_t bootstrap,
                        uint64_t seed, double* logz /*[nsamples]*/, double* info /*[nsamples]*/,
                        double* tip /*[nsamples * nfreq]*/, int64_t block_bytes, rvll_fip_merged_timing* timing);

/* ---- marginal histograms of the merged run's replicates (post-processing; independent of any model handle) ------- */
/* Per replicate s of rvll_merge_replicates (same seeds, multiplicities and merged order) the posterior mass of every bin of a
 * list of one- and two-dimensional histograms of the columns of values [n_rows, n_cols] (row-major, in input row order), and per
 * bin the statistics of that mass over the replicates (evidence_amd/marginals.py is the definition).  Axis a is the
 * column axis_col[a] with the edges edges[axis_edge_start[a] .. axis_edge_start[a + 1]) (2 to 4097 of them, finite, strictly
 * increasing).  The bin of x is numpy's histogram's: #{edges <= x} - 1, x equal to the last edge in the last bin, x below the
 * first or above the last edge outside.  Panel t has the axes panel_axes[2 t] and panel_axes[2 t + 1] (-1: one-dimensional; else
 * its bins are row-major with the first axis the major index; a row outside either axis is outside the panel) and at most 4096
 * bins, which are panel_start[t] .. panel_start[t + 1] of one flat array of nbins bins, panel after panel.
 * counts[b]: the rows in bin b; outside_count[t]: the rows outside panel t.  With p_i = exp(logwt_i) (0 for a row without
 * weight), m_i = rint(p_i 2^62) as int64 and M = sum m:  mass = (double)(sum of m_i over the rows of the bin) / (double)M and
 * the same for a panel's outside rows; NaN throughout a replicate with M = 0 (a bootstrap of empty runs).  Every sum over rows
 * is an integer sum.  stats[k * nbins + b], k = 0 .. 3: mean, standard deviation (ddof 0), minimum and maximum of mass over the
 * replicates that are not NaN, by a sequential Welford update in replicate order (NaN where there is none).  mass
 * [nsamples * nbins] and outside [nsamples * n_panels] may each be NULL.  logz[s], info[s] as rvll_merge_replicates gives them.
 * block_bytes bounds the bin table (2 * n_rows * n_axes bytes) plus, a replicate, its weights and its histograms
 * (8 * (n_rows + nbins + n_panels) bytes); 0 stands for the table plus 8 GiB, of which only nsamples replicates are allocated.
 * RVLL_E_NOMEM before any work when the table and one replicate do not fit.  The results do not depend on the batching, on the
 * other replicates or on the other panels of the call.
 * RVLL_E_INVALID: everything rvll_merge_replicates refuses; n_cols outside [1, 64], n_axes outside [1, 128], n_panels outside
 * [1, 256], an axis with fewer than 2 or more than 4097 edges, edges that are not finite or do not strictly increase, a panel of
 * more than 4096 bins, an axis or column index out of range, a value that is not finite, null required buffers.  timing may be
 * NULL.  device < 0 uses the current device. */
typedef struct rvll_marginal_timing {
    double  kernel_ms;       /* HIP-event time of all device work: setup_ms + weights_ms + reduce_ms                       */
    double  total_ms;        /* the whole call: checks, allocation, uploads, kernels, downloads                            */
    double  setup_ms;        /* the merge's setup, the bin table and the counts                                            */
    double  weights_ms;      /* the replicate kernels (what rvll_merge_replicates spends on the same input)                 */
    double  reduce_ms;       /* fixed point, the histogram kernel and the statistics                                       */
    int64_t rows;            /* n_rows                                                                                      */
    int64_t elements;        /* (row, replicate) pairs: n_rows * nsamples                                                   */
    int64_t bins;            /* nbins: the bins of all panels together                                                      */
    int32_t launches;        /* 6 for the setup, then 4 a block of replicates (a rocPRIM sort counted as one)               */
    int32_t threads;         /* per workgroup of the histogram kernel                                                       */
    int32_t blocks;          /* blocks of replicates the call was split into                                                */
    int32_t groups;          /* panel groups: each is one pass over a replicate's weights                                   */
} rvll_marginal_timing;
int rvll_marginal_replicates(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                             const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs,
                             const double* values /*[n_rows * n_cols]*/, int32_t n_cols, const double* edges,
                             const int32_t* axis_col /*[n_axes]*/, const int64_t* axis_edge_start /*[n_axes + 1]*/,
                             int32_t n_axes, const int32_t* panel_axes /*[2 * n_panels]*/, int32_t n_panels, int32_t nsamples,
                             int32_t mode, int32_t bootstrap, uint64_t seed, double* logz /*[nsamples]*/,
                             double* info /*[nsamples]*/, int64_t* counts /*[nbins]*/, int64_t* outside_count /*[n_panels]*/,
                             double* stats /*[4 * nbins]*/, double* mass /*NULL or [nsamples * nbins]*/,
                             double* outside /*NULL or [nsamples * n_panels]*/, int64_t block_bytes,
                             rvll_marginal_timing* timing);

/* ---- equal-weight draws of the merged run's replicates (post-processing; independent of any model handle) --------- */
/* Per replicate s of rvll_merge_replicates (same seeds, multiplicities and merged order) ndraws rows drawn by systematic
 * resampling with one uniform (evidence_amd/draws.py is the definition).  With m_i = rint(exp(logwt_i) 2^62) as int64
 * (0 for a row without weight; the integers of rvll_marginal_replicates), C the inclusive running sum of m in merged order,
 * M its last entry, U the 53-bit integer behind uniform01 of (seed_s ^ 0xA0761D6478BD642F, 0), Q = M / ndraws (integer) and
 * O = (U Q) >> 53:  tau_k = k Q + O, and draw k is the first merged row with C > tau_k.  rows[s * ndraws + k] is that row's
 * input row, ascending in merged order over k; a row is drawn floor or ceil of ndraws p_i times, a row with m = 0 never; a
 * replicate with M < ndraws (a bootstrap of empty runs) has -1 throughout.  logz[s], info[s] as rvll_merge_replicates gives
 * them.  fixed [nsamples * n_rows] (m in merged order) and msum [nsamples] (M) may each be NULL.  block_bytes bounds the device
 * block of weights (8 * n_rows bytes a replicate); 0 stands for 8 GiB, of which only nsamples replicates are allocated;
 * RVLL_E_NOMEM before any work when one replicate does not fit.  Every decision is an integer comparison: the results do not
 * depend on the batching or on the other replicates.  RVLL_E_INVALID: everything rvll_merge_replicates refuses, ndraws outside
 * [1, 2^20], null required buffers.  timing may be NULL.  device < 0 uses the current device. */
typedef struct rvll_draw_timing {
    double  kernel_ms;       /* HIP-event time of all device work: setup_ms + weights_ms + reduce_ms                       */
    double  total_ms;        /* the whole call: checks, allocation, uploads, kernels, downloads                            */
    double  setup_ms;        /* the merge's setup                                                                           */
    double  weights_ms;      /* the replicate kernels (what rvll_merge_replicates spends on the same input)                 */
    double  reduce_ms;       /* scan_ms + pick_ms, and the download of `fixed` when it is asked for                         */
    double  scan_ms;         /* fixed point and the three launches of the running sum                                       */
    double  pick_ms;         /* the searches                                                                                */
    int64_t rows;            /* n_rows                                                                                      */
    int64_t elements;        /* (row, replicate) pairs: n_rows * nsamples                                                   */
    int64_t draws;           /* ndraws * nsamples                                                                           */
    int32_t launches;        /* 4 for the setup, then 6 a block of replicates (a rocPRIM sort counted as one)               */
    int32_t threads;         /* per workgroup                                                                               */
    int32_t blocks;          /* blocks of replicates the call was split into                                                */
    int32_t tiles;           /* tiles of 1024 rows of the running sum                                                       */
} rvll_draw_timing;
int rvll_draw_replicates(int32_t device, const double* logl /*[n_rows]*/, const double* birth /*[n_rows]*/, int64_t n_rows,
                         const int64_t* run_start /*[n_runs + 1]*/, int32_t n_runs, int32_t ndraws, int32_t nsamples,
                         int32_t mode, int32_t bootstrap, uint64_t seed, int32_t* rows /*[nsamples * ndraws]*/,
                         double* logz /*[nsamples]*/, double* info /*[nsamples]*/, int64_t* fixed /*NULL or [nsamples * n_rows]*/,
                         int64_t* msum /*NULL or [nsamples]*/, int64_t block_bytes, rvll_draw_timing* timing);

/* ---- MLFriends region sampling (evidence_amd/region.py holds the definition) -----------------------------------
 * kdraw draws from the constrained prior of each of R runs by uniform rejection sampling from the union of the balls of
 * radius2[r] (in the metric scale[r], as rvll_cluster_runs takes and returns them) around the run's survivors (rows
 * run_start[r] .. run_start[r + 1] of `survivors`, unit-cube rows).  Candidates are numbered first, first + 1, ..., at most
 * max_candidates of them a run; every random number of candidate c is uniform01(seeds[r], c << 8 | draw), so a candidate does
 * not depend on the block, the round or the call that handles it.  Candidate c: a centre row, an offset uniform in the ball
 * (the walk's normals), wrapped dimensions folded, any other dimension outside [0, 1) flags it RVLL_REGION_OUTSIDE; n = the
 * survivors within radius2 (n = 0: RVLL_REGION_LOST); kept iff U n < 1; kept candidates get theta and log-L from the prior and
 * log-L kernels of rvll_prior_loglike_batch (the same bits); accepted iff log-L > lstar[r].  In rounds, every run that is still
 * short proposes `block` candidates (1 .. 2^20); a run's points are its first kdraw accepted candidates in candidate order:
 * cube_out / theta_out [R, kdraw, ndim], logl_out [R, kdraw] (rows past nfound[r]: NaN), ncalls[r] = the kept candidates up to
 * the last one taken (all kept ones when nfound[r] < kdraw).  A run without survivors, or whose ball meets its own image in a
 * wrapped dimension (sqrt(radius2) / scale >= 0.5), draws nothing.  The results do not depend on block or on the other runs.
 * Trace (trace_cap > 0, else the pointers may be NULL): per run the first trace_cap candidates it evaluated, trace_count[r] of
 * them: cube [R, trace_cap, ndim], flags, n, log-L (NaN where not kept).  rounds (may be NULL): the rounds the call took.
 * rvll_region_tile_rows: the survivors one LDS image holds at ndim parameters (more are counted tile by tile).
 * Needs rvll_set_priors (RVLL_E_NOPRIORS).  RVLL_E_INVALID: run_start not rising from 0, a scale that is not finite and
 * positive, a radius2 that is not finite and non-negative, a NaN lstar, kdraw / first / max_candidates negative, block out of
 * range, a required pointer NULL; RVLL_E_UNSUPPORTED: ndim above 64; RVLL_E_NOMEM: more than 4 GiB of device work space.   */
#define RVLL_REGION_OUTSIDE  1
#define RVLL_REGION_LOST     2
#define RVLL_REGION_KEPT     4
#define RVLL_REGION_ACCEPTED 8
int rvll_region_draw_runs(rvll_handle* h, const double* survivors /*[N, ndim]*/, const int64_t* run_start /*[R + 1]*/, int64_t R,
                          const double* scale /*[R, ndim]*/, const double* radius2 /*[R]*/, const double* lstar /*[R]*/,
                          const uint64_t* seeds /*[R]*/, const int32_t* wrapped /*NULL or [ndim]*/, int32_t kdraw, int64_t first,
                          int64_t max_candidates, int32_t block, double* cube_out, double* theta_out, double* logl_out,
                          int32_t* nfound /*[R]*/, int64_t* ncalls /*[R]*/, int64_t trace_cap, double* trace_cube,
                          int32_t* trace_flags, int32_t* trace_n, double* trace_logl, int64_t* trace_count /*[R]*/,
                          int32_t* rounds);
int rvll_region_tile_rows(int32_t ndim, int32_t* rows);

/* ---- diagnostics -------------------------------------------------------------- */
/* Evaluate one device math routine elementwise (tests only; no reference counterpart):
 * op 0 sin, 1 cos (rvll sincos), 2 div_exact(x,y), 3 x/y (IEEE), 4 div_fast(x,y),
 * 5 log_pos(x), 6 library log(x), 7 ndtri(x), 8/9 sin/cos after rotate_small by y, 10 div_1nr, 11 v_rcp_f64,
 * 12/13 the wave reduction tree by shuffles / by permlane-swap + DPP (lane 0 of every 64 values), 14 the Cephes
 * form of ndtri (scipy's routine; op 7 is AS241), 15 - 19 latency chains, 20/21 sin/cos of sincos_cr,
 * 22/23 sin/cos of sincos_any, 24/25 reduce_huge: r and q mod 4 (|x| >= 2^-10, finite; nan elsewhere).
 * The fp32 layer, floats cast in and widened out: 26/27 sincos_f32, 28 - 31 sincos_f32x2 on (x, y): s.x, s.y, c.x, c.y,
 * 32 reduce_2pi_to_f32, 33 div_f32(x, y), 34/35 div_f32x2 of (x, 3 x) by (y, 2 - y): .x, .y.
 * The rotation between Newton steps: 36/37 sin/cos of the pair sincos(x) after rotate_mid by y (|y| <= pi/4).
 * The Newton step's residuals: 38/39 f / f' of newton_residuals; x holds records (E, s, c, e, M) of five doubles, y is not
 * read, the result stands at the record's first element (nan at the other four).
 * The shortcut solve from E = M at tol 1e-4: x holds n / 2 records (M, e) of two doubles, y is not read, record i is lane i's and
 * its result stands at out[i] (nan from n / 2 on): 40/41/42 s, c, dE as the solve leaves them and 43 whether it settled within
 * eight steps (1 / 0), first trip compiled and the later ones hand-written (newton_trips_asm); 44 - 47 the same by the compiled
 * loop throughout.   */
int rvll_debug_eval(rvll_handle* h, int32_t op, const double* x, const double* y,
                    int64_t n, double* out);

/* One launch of a stamped twin of the fp64 log-L kernel over the resident theta (after `warmup` ordinary
 * launches): per workgroup 8 words — [0] start, [1] per-point decode done, [2..5] item loop done per wave,
 * [6] end (constant 100 MHz clock), [7] HW_ID | XCC_ID << 32.  out == NULL only returns the geometry.  The
 * stamps never execute in the product kernels (no reference counterpart; profiles/ records are made with it). */
int rvll_dev_trace_loglike(rvll_handle* h, int64_t B, int32_t warmup, uint64_t* out, int64_t out_words,
                           int32_t* blocks, int32_t* points_per_block);

/* The exact redo of wandering Kepler solves (round 4; default on; RVLL_WANDER_EXACT=0 in the environment at rvll_create turns it
 * off).  Started at E = M next to a zero of 1 - e cos E (e >= 0.97) the reference's Newton iteration wanders for 30 - 350 steps,
 * and where it stops hangs on the last bit of every sin / cos on the way.  With the switch on, a solve that takes
 * more than eight steps is done again from its start with correctly rounded sin / cos — what glibc's are nearly always — and
 * the device is within 1e-10 of the reference on all but ~0.01 % of points with a planet at e >= 0.97 (1.4 % without; the
 * points still carry RVLL_FLAG_WANDERED).  Costs nothing where no solve wanders.  The proposal walk evaluates its CANDIDATES
 * without the redo (a wandering solve would hold a whole round up) and puts the log-L of the points it ENDS on right.   */
int rvll_set_wander_exact(rvll_handle* h, int32_t on);
/* The kernels that carry a log-L tile next to the prior stage (one-launch cube -> log-L, the walk) evaluate Beta /
 * Gamma quantiles by their verified tables over |logit q| <= umax (default: the whole table, 30) and hand every
 * other element to the routines with the full solvers — same results either way.  Lowering umax (0: nothing is
 * taken by the tables) exists so that tests can drive that hand-over; no reference counterpart.               */
int rvll_set_slim_table_range(rvll_handle* h, double umax);

/* ---- housekeeping ---------------------------------------------------------- */
const char* rvll_last_error(void);
int rvll_version(int32_t* major, int32_t* minor);
int rvll_device_count(int32_t* count);
int rvll_device_name(int32_t device, char* buf, int32_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* RVLL_H */
