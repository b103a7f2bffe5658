/* include/spg.h — C ABI of the MI355X pose-graph sparsification hot path.
 *
 * The reference (Lecanyu/SparsifyPoseGraph) has no FFI: its seams are C++ virtual interfaces.
 * Each entry point below names the reference interface it stands in for (file:line under the
 * reference tree). The product library libspg_hip.so exports every symbol declared here; the CPU
 * oracle (oracle/libspg_ref.so, test infrastructure only) exports spg_marginalize_batch and
 * spg_run_round with the same signatures so parity tests call both through one binding.
 *
 * Conventions: plain pointers and sizes; caller owns every buffer it passes; the library owns the
 * context/graph objects it returns. All arithmetic is fp64, graph indices int32, arena offsets int64
 * (counted in doubles). Functions return 0 on success or a negative SPG_E* code; they never abort.
 */
#ifndef SPG_H_
#define SPG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums mirroring reference types ------------------------------------------------------- */
/* EvaluateInfo::algorithm (src/evaluate.h:20-22) / GraphWrapperG2O(useGLC) (src/graph_wrapper_g2o.cpp:102) */
enum { SPG_ALG_NFR = 0, SPG_ALG_GLC = 1 };
/* SparsityOptions::SparsityTopology (src/sparsity_options.h:12-14), same numeric order */
enum { SPG_TOPO_TREE = 0, SPG_TOPO_SUBGRAPH = 1, SPG_TOPO_CLIQUEY_SUBGRAPH = 2, SPG_TOPO_DENSE = 3,
       SPG_TOPO_CLIQUEY_DENSE = 4 };
/* SparsityOptions::LinearizationPoint (src/sparsity_options.h:16-18) */
enum { SPG_LIN_LOCAL = 0, SPG_LIN_GLOBAL = 1 };
/* edge kinds: pose-pose edge (EdgeSE2ISAM / EdgeSE3ISAM, src/se2_compatibility.h:20, src/se3_compatibility.h:25)
 * and n-ary GLC edge (GLCEdge, src/glc_edge.h:14) */
enum { SPG_EDGE_BINARY = 0, SPG_EDGE_GLC = 1, SPG_EDGE_MULTI = 2 };
/* SPG_EDGE_MULTI = MultiEdgeCorrelated<EdgeSE2 | EdgeSE3> (src/multi_edge_correlated.hpp:28-140): nm pose-pose measurements
 * between pairs of the edge's q vertices with ONE joint information matrix Omega (d nm x d nm), what the CliqueySubgraph /
 * CliqueyDense patterns emit (src/topology_provider_binary.hpp:48-67). Record (doubles):
 *   [0] nm | [1 + 2 i], [2 + 2 i]: the two vertices of measurement i as indices into the edge's vertex list |
 *   nm measurements (3 | 7 each) | W (r x r row-major, r = d nm) with Omega = W^T W.
 * The error is the stack of the pose-pose errors; chi2 = || W e ||^2. */
#define SPG_MULTI_LEN(d, nm) (1 + 2 * (nm) + (nm) * ((d) == 3 ? 3 : 7) + (int64_t)(d) * (nm) * (d) * (nm))

/* per-blanket status (replaces the reference's assert / exit(0) / NULL-edge failure modes,
 * src/vertex_remover.cpp:291,461, src/optimizer.cpp:75-77, src/topology_provider_glc.cpp:46-49,85-89) */
enum {
    SPG_OK = 0,
    SPG_ST_HMM_NOT_PD = 1,      /* LLT(H_mm) failed (src/vertex_remover.cpp:444) */
    SPG_ST_EIG_FAIL = 2,        /* eigen-decomposition did not converge */
    SPG_ST_NONFINITE = 3,       /* non-finite value in the target information */
    SPG_ST_TIKHONOV_NOT_PD = 4, /* LLT(Lambda + I) failed (src/pseudo_chow_liu.cpp:189) */
    SPG_ST_CLOSED_FORM_NOT_PD = 5, /* LLT(J Sigma J^T) failed (src/logdet_function.cpp:246,273) */
    SPG_ST_KLD_NOT_PD = 6,      /* value() returned +inf (src/logdet_function.cpp:130-131); edges still valid */
    SPG_ST_NEEDS_INTERIOR_POINT = 7, /* no closed form (src/optimizer.cpp:38-79): out of scope, no edges written */
    SPG_ST_MARGINAL_NOT_PD = 8, /* LLT inside PseudoChowLiu::marginal failed (src/pseudo_chow_liu.cpp:134) */
    SPG_ST_EMPTY_BLANKET = 9,   /* removed vertex without edges (assert at src/vertex_remover.cpp:291) */
    SPG_ST_UNSUPPORTED = 10,    /* option combination the reference asserts against or that is out of scope */
    SPG_ST_NEEDS_LOCAL_OPTIMIZATION = 11 /* Local linearisation point without a closed-form estimate where the 10 LM iterations of
                                   src/vertex_remover.cpp:382-391 cannot run: a blanket that holds a GLC edge (the GLC provider
                                   asserts the Global point, src/topology_provider_glc.cpp:110-111). Pose-pose and correlated
                                   blankets of every NFR pattern, clusters included, are re-linearised on the device. */
};
/* informational bits OR-ed into status << 8 are not used; see spg_result.info */
enum {
    SPG_INFO_RANK_DEFICIENT = 1, /* smalleigs > dim: chooseDimensions path taken (src/logdet_function.cpp:42-59) */
    SPG_INFO_GLC_ROOT_EDGE = 2,  /* a unary GLC root edge survived the 1e-8 cut (src/topology_provider_glc.cpp:134-140) */
    SPG_INFO_IP_HESSIAN_NOT_PD = 4, /* interior point: a Newton system was not positive definite and that barrier step was given up
                                    (src/pqn/pqn_optimizer.cpp:48-53 solves with the failed LLT unchecked; the loop over rho,
                                    src/optimizer.cpp:60-75, goes on from the same x either way) */
    SPG_INFO_GLC_KLD_SKIPPED = 8, /* SPG_FLAG_GLC_KLD was set, but the per-blanket KLD of this GLC blanket is not defined by the
                                    gauge route and stays NaN: trace(C^-1) >= 5e4 (the NFR route's guard), the tail cut an
                                    eigenvalue of the target (the edges carry fewer than n - d rows), a root edge was emitted, a
                                    Cholesky factorisation failed, or the blanket took the large-blanket pipeline */
    SPG_INFO_FD_MAX_CYCLES = 16 /* SPG_FLAG_NFR_FACTOR_DESCENT: the descent of this blanket ended at max_cycles, not at the stop rule
                                    (always so when spg_ctx_set_factor_descent asked for a fixed number of cycles). Not an error:
                                    every cycle lowers the KLD, and the edges are those of the last cycle. */
};

enum {
    SPG_EINVAL = -1, SPG_ENODEV = -2, SPG_ENOMEM = -3, SPG_ECAPACITY = -4, SPG_EHIP = -5, SPG_EIO = -6,
    SPG_ESTATE = -7, SPG_EBLANKET = -8, /* at least one blanket has status != OK that prevents graph update */
    SPG_ENOTPD = -9 /* a graph's information matrix is not positive definite (global KLD) */
};

/* SparsityOptions (src/sparsity_options.h:11-30) + algorithm selector + pose dimension */
typedef struct {
    int32_t pose_dim;             /* 3 (SE2) or 6 (SE3) */
    int32_t algorithm;            /* SPG_ALG_* */
    int32_t topology;             /* SPG_TOPO_* */
    int32_t lin_point;            /* SPG_LIN_* */
    int32_t include_intra_clique; /* reference default true; never changed by any caller */
    int32_t flags;                /* SPG_FLAG_* */
    double chord_ratio;           /* reference default 1 */
} spg_options;
enum {
    SPG_FLAG_RESERVED0 = 1, /* bit 0 is reserved (the oracle uses it for a private GLC diagnostic) */
    SPG_FLAG_FORCE_EIG = 2, /* always take the eigen-decomposition route of src/logdet_function.cpp:14-64
                               (default: the equivalent gauge/Cholesky route whenever its guard holds) */
    SPG_FLAG_GLC_KLD = 4,   /* GLC only: also compute the per-blanket KLD of every removal (the reference's GLC provider has no
                               LogdetFunction and reports none). With A = sum_e (W_e G_e)^T (W_e G_e) over the emitted edges (G_e =
                               the reparametrisation Jacobian), N^ the orthonormal gauge basis and C = Lambda_t + N^ N^^T:
                                   kld = 1/2 (tr(C^-1 A) - log det(A + N^ N^^T) + log det C - (n - d)),
                               src/logdet_function.cpp:119-133 at the GLC edges' information, the NFR branch's gauge route.
                               Edges and statuses are bit-identical to an unflagged run; the value lands after the ready word,
                               like the NFR one. Where it is not defined the blanket reports NaN + SPG_INFO_GLC_KLD_SKIPPED;
                               the large-blanket pipeline (GLC Dense beyond the LDS kernel) never computes it. Backends other
                               than the HIP one may ignore the flag. Clear (default): kld stays NaN for GLC. */
    SPG_FLAG_NFR_FACTOR_DESCENT = 8,
                            /* NFR only, and only the blankets whose pattern is uncorrelated with more than k - 1 edges (Subgraph,
                               Dense): the ones the interior point of src/optimizer.cpp:38-79 takes. Their informations come from
                               factor descent instead (Vallve, Sola, Andrade-Cetto, RA-L 2018): cyclic block-coordinate descent
                               on the same convex problem, min KLD(X) over the edge informations. With J~_e = J_e U, S the
                               spectrum of the target, T_e = J~_e S J~_e^T, M = sum_e J~_e^T X_e J~_e and P = M^-1: start at
                               X_e = T_e^-1; a cycle visits the edges in pattern order and sets, with A = J~_e P J~_e^T,
                               Psi = A^-1 - X_e, T_e = L L^T and sym(L^T Psi L) = V diag(psi) V^T,
                                   X_e <- L^-T V diag(max(1 - psi_i, 1e-9)) V^T L^-1,
                               the exact minimiser over X_e >= 1e-9 T_e^-1 with the other edges fixed (every information stays
                               positive definite). M is factorised afresh after every cycle; the run stops after the first cycle
                               whose KLD decrease is <= rel_tol max(1, |KLD|) or after max_cycles (spg_ctx_set_factor_descent;
                               SPG_INFO_FD_MAX_CYCLES). The cycle count lands in info >> 8, where the interior point reports its
                               Newton steps. A T_e that is not positive definite: SPG_ST_CLOSED_FORM_NOT_PD, no edges; an M that
                               is not: SPG_ST_KLD_NOT_PD and the edges of the last completed cycle. No Newton system, so no limit
                               on d^2 E: k <= 256 as for the closed forms. Every other blanket (Tree and correlated patterns,
                               tree-shaped Subgraph blankets, GLC) is bit-identical to an unflagged run. Backends other than the
                               HIP one may ignore the flag. Clear (default): the interior point. */
    /* bits 8..15: diagnostic pipeline truncation used by tools/phase_bench.py */
};

/* One batch of mutually independent Markov blankets in CSR form: the data VertexRemover::remove
 * gathers per iteration (src/vertex_remover.cpp:93-108): blanket vertices (removed first, then kept
 * in ascending original id = g2o indexMapping order, src/vertex_remover.cpp:349-356), their
 * estimates, and every edge with all endpoints in the blanket (src/vertex_remover.cpp:225-251). */
typedef struct {
    int32_t B;
    const int32_t *vert_off;      /* B+1 */
    const int32_t *n_remove;      /* B : m_b >= 1 */
    const int32_t *vert_id;       /* V : original ids (only echoed into new_edge_vert) */
    const double *pose;           /* V x (3 | 7): (x y theta) | (tx ty tz qx qy qz qw) */
    const int32_t *edge_off;      /* B+1 */
    const int32_t *edge_kind;     /* E : SPG_EDGE_* */
    const int32_t *edge_vert_off; /* E+1 */
    const int32_t *edge_vert;     /* local vertex index inside the blanket */
    const int64_t *edge_data_off; /* E+1 */
    const double *edge_data;      /* binary: meas (3|7) + information upper triangle row-wise (6|21)
                                     GLC   : meas (d*q) + W row-major (r x d*q)  [r = (len-dq)/dq] */
} spg_batch;

/* Outputs of VertexRemover::remove for the batch: the new edges handed to updateInputGraph
 * (src/vertex_remover.cpp:500-546), plus the target information (src/vertex_remover.cpp:447-449)
 * and the per-blanket KLD (src/logdet_function.cpp:119-133). Capacities are supplied by the caller. */
typedef struct {
    double *target_info;          /* optional (NULL to skip): blanket b at target_info_off[b], n_b x n_b row-major */
    const int64_t *target_info_off; /* B+1 when target_info != NULL */
    int32_t *new_edge_off;        /* B+1, written */
    int32_t *new_edge_kind;       /* new_edge_cap */
    int32_t *new_edge_vert_off;   /* new_edge_cap+1 */
    int32_t *new_edge_vert;       /* ORIGINAL ids, new_edge_vert_cap */
    int64_t *new_edge_data_off;   /* new_edge_cap+1 */
    double *new_edge_data;        /* same record layout as spg_batch.edge_data */
    int32_t new_edge_cap, new_edge_vert_cap;
    int64_t new_edge_data_cap;
    double *kld;                  /* B : NFR: always (closed-form blankets); GLC: NaN unless SPG_FLAG_GLC_KLD is set */
    double *min_gap;              /* B, optional: smallest relative gap between consecutive Chow-Liu weights popped */
    int32_t *status;              /* B : SPG_ST_* */
    int32_t *info;                /* B, optional: SPG_INFO_* bits */
} spg_result;

/* ---- context ------------------------------------------------------------------------------ */
typedef struct spg_ctx spg_ctx;
/* one context per (host thread, device); owns a HIP stream and scratch. device = HIP ordinal.
 * Fails with SPG_ENODEV when no gfx950 device / code object is available: there is no CPU fallback. */
int spg_ctx_create(spg_ctx **out, int device);
/* Multi-GPU form (the reference has no counterpart: one process, no collective): one process per
 * GPU, rank r of nranks. nccl_unique_id = the SPG_UNIQUE_ID_BYTES bytes rank 0 obtained from spg_get_unique_id and
 * handed to every rank (any out-of-band channel: a file, MPI, torch.distributed's store); the call runs
 * ncclCommInitRank (RCCL, bound from librccl.so.1 at this call — single-GPU users never load it) and is
 * collective over the ranks. NULL id: no communicator (exchange through the caller's callback, or a single rank). */
#define SPG_UNIQUE_ID_BYTES 128
int spg_get_unique_id(void *id_out /* SPG_UNIQUE_ID_BYTES */);
int spg_ctx_create_ranks(spg_ctx **out, int device, int rank, int nranks, const void *nccl_unique_id);
int spg_ctx_rank(const spg_ctx *ctx);
int spg_ctx_nranks(const spg_ctx *ctx);
/* The built-in exchange of one sharded round: in-place ncclAllGather of the nranks equal chunks of
 * arena[region_off, region_off + nranks*chunk_len) (doubles; rank r owns chunk r) over RCCL / xGMI, on the
 * context's stream, then a stream synchronisation. What spg_graph_marginalize_ranks does per exchanged batch when
 * no callback is given. No-op for a context without a communicator. */
int spg_allgather_region(spg_ctx *ctx, void *arena, int64_t region_off, int64_t chunk_len);
void spg_ctx_destroy(spg_ctx *ctx);
const char *spg_last_error(spg_ctx *ctx);
/* HIP stream the context launches on (hipStream_t as void*), for event timing by the caller */
void *spg_ctx_stream(spg_ctx *ctx);
int spg_ctx_synchronize(spg_ctx *ctx);
/* per-launch timing of the blanket kernel with HIP events on the context stream (bench roofline leg):
 * enable/reset, then read the sums over the timed launches completed since: kernel milliseconds,
 * algorithmic HBM bytes (SURVEY.md 8d formula evaluated on the launched blankets), launches, blankets.
 * enable = 1 times every launch (what bench.py uses); enable = n > 1 only every n-th one; 0 switches timing
 * off. (Sampling does not pay on ROCm 7.2: launches without the trailing event record were measured to
 * cost more host time than the two records they save.) */
int spg_ctx_profile(spg_ctx *ctx, int enable);
int spg_ctx_profile_read(spg_ctx *ctx, double *kernel_ms, double *alg_bytes, int64_t *launches, int64_t *blankets);
/* the same for the persistent worker kernel (narrow batches are handed to one long-lived kernel per marginalisation
 * instead of being launched one by one): its runs, their total duration (HIP events around the kernel), the
 * algorithmic bytes and blankets it processed. Not included in spg_ctx_profile_read. */
int spg_ctx_profile_read_worker(spg_ctx *ctx, double *kernel_ms, double *alg_bytes, int64_t *runs, int64_t *blankets);
/* and for the large-blanket pipeline (GLC Dense blankets beyond the LDS kernel's capacity run dense in HBM on the fp64
 * matrix cores): blankets processed since the last spg_ctx_profile call, their total device time (HIP events), the
 * n^3-class flops of their factorisations, the largest (k + m) * pose_dim seen. */
int spg_ctx_profile_read_big(spg_ctx *ctx, double *kernel_ms, double *flops, int64_t *blankets, int32_t *n_max);

/* VertexRemover::remove restricted to its arithmetic, for B independent blankets at once
 * (replaces src/vertex_remover.cpp:108-132 + src/topology_provider_binary.hpp:23-70 +
 *  src/topology_provider_glc.cpp:100-185 + src/optimizer.cpp:16-22). Host pointers. */
int spg_marginalize_batch(spg_ctx *ctx, const spg_options *opts, const spg_batch *batch, spg_result *result);

/* ---- decimation (src/decimation.h:18-22, src/decimation.cpp:11-49) -------------------------- */
/* Each writes at most cap ids into out and returns the count (or the required count if > cap). */
int spg_decimate_global(int last, int endvert, int sparsity, int cluster_size, int32_t *out, int cap);
int spg_decimate_online(int last, int endvert, int sparsity, int cluster_size, int32_t *out, int cap);
int spg_decimate_cluster(int last, int endvert, int sparsity, int cluster_size, int32_t *out, int cap);

/* ---- device-resident graph: GraphWrapper (src/graph_wrapper.h:17-78) ------------------------- */
typedef struct spg_graph spg_graph;

/* GraphWrapperG2O(verbose,useGLC) (src/graph_wrapper_g2o.cpp:102): empty graph of SE2 (3) or SE3 (6) poses */
int spg_graph_create(spg_ctx *ctx, int pose_dim, spg_graph **out);
void spg_graph_destroy(spg_graph *g);
/* GraphWrapperG2O(fname, optimize=false, ...) (src/graph_wrapper_g2o.cpp:107-154), .g2o text:
 * VERTEX_SE2 / EDGE_SE2 / VERTEX_SE3:QUAT / EDGE_SE3:QUAT and GLC_EDGE (src/glc_edge.cpp:65-93). The estimates
 * are taken as stored (optimize=false); call spg_graph_optimize for the reference's optimize=true. */
int spg_graph_load_g2o(spg_ctx *ctx, const char *path, spg_graph **out);
/* GraphWrapper::write (src/graph_wrapper_g2o.cpp:467-470) incl. GLC_EDGE records (src/glc_edge.cpp:95-119) */
int spg_graph_write_g2o(spg_graph *g, const char *path);
/* GraphWrapper::write(std::ofstream &) (src/graph_wrapper.h:62): the same text into a malloc'ed buffer
 * (*text, *len bytes, NUL-terminated); release it with spg_free. */
int spg_graph_write_g2o_mem(spg_graph *g, char **text, size_t *len);
void spg_free(void *p);
/* GraphWrapperG2O::clonePortion(maxid) (src/graph_wrapper_g2o.cpp:334-356): a new graph on the same context with
 * the vertices of id <= maxid (estimates copied) and the edges whose endpoints all satisfy it. The reference then
 * calls optimize() on the clone; here that is the caller's next call (spg_graph_optimize). */
int spg_graph_clone_portion(spg_graph *g, int maxid, spg_graph **out);
/* GraphWrapperG2O::covariance() (src/graph_wrapper_g2o.cpp:368-373): inverse of spg_graph_information, dense on
 * the device (blocked fp64-MFMA Cholesky, triangular inverse, L^-T L^-1). Same conventions as
 * spg_graph_information: returns n; the n x n row-major matrix is written if cap >= n*n. */
int64_t spg_graph_covariance(spg_graph *g, int32_t fixed_id, double *out, int64_t cap);
/* GraphWrapper::Vertex::edges() (src/graph_wrapper.h:26): indices (into the order of spg_graph_get_edges) of the
 * live edges incident to vertex id, ascending. Returns the count (writes at most cap). */
int spg_graph_vertex_edges(spg_graph *g, int id, int32_t *edge_index, int cap);
/* addVertex / addEdge (src/graph_wrapper_g2o.cpp:214-247). pose/meas as in spg_batch; info = upper triangle */
int spg_graph_add_vertex(spg_graph *g, int id, const double *pose);
int spg_graph_add_edge(spg_graph *g, int from, int to, const double *meas, const double *info_upper);
/* bulk forms: poses n x (3|7); ij n x 2; records n x (meas + info upper triangle) */
int spg_graph_add_vertices(spg_graph *g, int n, const int32_t *ids, const double *poses);
int spg_graph_add_edges(spg_graph *g, int n, const int32_t *ij, const double *records);
/* n-ary GLC edge (GLCEdge::read, src/glc_edge.cpp:64-93) */
int spg_graph_add_glc_edge(spg_graph *g, int q, const int32_t *ids, int r, const double *meas, const double *W);
/* MultiEdgeCorrelated over q vertices (src/multi_edge_correlated.hpp:28-63): `record` in the SPG_EDGE_MULTI layout above,
 * len = SPG_MULTI_LEN(pose_dim, nm). */
int spg_graph_add_multi_edge(spg_graph *g, int q, const int32_t *ids, const double *record, int64_t len);
int spg_graph_pose_dim(const spg_graph *g);
int spg_graph_num_vertices(const spg_graph *g);
int spg_graph_num_edges(const spg_graph *g);
int64_t spg_graph_edge_data_size(const spg_graph *g); /* total doubles of all live edge records */
int64_t spg_graph_edge_vert_size(const spg_graph *g); /* total endpoints of all live edges */
/* vertices() / vertex(id)->estimate() (src/graph_wrapper.h:70-72): ids ascending, poses V x (3|7) */
int spg_graph_get_vertices(spg_graph *g, int32_t *ids, double *poses);
/* all live edges in insertion order; arrays sized from the three counters above (+1 for offsets) */
int spg_graph_get_edges(spg_graph *g, int32_t *kind, int32_t *vert_off, int32_t *vert_ids,
                        int64_t *data_off, double *data);
/* setEstimate (src/graph_wrapper_g2o.cpp:614-621) */
int spg_graph_set_estimate(spg_graph *g, int id, const double *pose);

typedef struct {
    int32_t n_removed;     /* vertices actually marginalised */
    int32_t n_rounds;      /* conflict-free rounds executed */
    int32_t n_new_edges;
    int32_t n_bad_status;  /* blankets with a status that is not SPG_OK / SPG_ST_KLD_NOT_PD */
    int32_t max_blanket;   /* largest k+m */
    int32_t n_launches;    /* kernel launches */
    double kld_sum;        /* sum of finite per-blanket KLD (GLC: 0 unless SPG_FLAG_GLC_KLD is set) */
    double host_seconds;   /* host scheduling + graph update */
    double device_seconds; /* time blocked on the device (launch -> results visible) */
    double schedule_seconds; /* part of host_seconds: conflict-free round selection */
    double commit_seconds;   /* part of host_seconds: graph update */
    double launch_seconds;   /* part of device_seconds: descriptor upload + kernel launch calls */
    int32_t n_batches;         /* batches of blankets handed to the device (a round may be cut into several) */
    int32_t n_exchanged;       /* batches that were sharded over the ranks and all-gathered */
    double exchange_seconds;   /* time inside the exchange (collective + its synchronisation) */
    double exchanged_bytes;    /* bytes all-gathered (whole regions, all ranks' chunks) */
} spg_marg_stats;

/* GraphWrapperG2O::marginalizeNoOptimize (src/graph_wrapper_g2o.cpp:398-453): removes `which` with
 * the sequential semantics of VertexRemover::remove (src/vertex_remover.cpp:83-140), executed as
 * conflict-free rounds of independent blankets on the device. Does NOT run optimize()
 * (src/graph_wrapper_g2o.cpp:462); GraphWrapperG2O::marginalize = this + spg_graph_optimize. */
int spg_graph_marginalize(spg_graph *g, const int32_t *which, int n, const spg_options *opts,
                          spg_marg_stats *stats);
/* The same call for nranks cooperating processes (one per GPU), each holding an identical replica:
 * batches below the shard threshold are computed redundantly by every rank (no communication);
 * a batch at or above it is sharded, and `exchange` is called once for it — it must all-gather the
 * nranks equal chunks of arena[region_off, region_off + nranks*chunk_len) in place (rank r owns
 * chunk r), e.g. ncclAllGather / torch.distributed.all_gather_into_tensor, and return 0. */
typedef int (*spg_exchange_fn)(void *user, void *arena, int64_t region_off, int64_t chunk_len, int nranks, int rank);
/* exchange == NULL with nranks > 1: the built-in RCCL all-gather of the graph's context (spg_ctx_create_ranks with
 * the same rank / nranks); a callback overrides it (tests: gloo, host staging). */
int spg_graph_marginalize_ranks(spg_graph *g, const int32_t *which, int n, const spg_options *opts, int rank, int nranks,
                                spg_exchange_fn exchange, void *exchange_user, spg_marg_stats *stats);
/* Which batches are sharded. Default policy (threshold < 0): a cost model — a batch is sharded when the modelled
 * device time of this rank's slice plus one exchange is below the modelled time of the whole batch on one GPU
 * (per-blanket chain latency ~ n^2.5, blankets resident per GPU from the LDS carve-up, exchange = latency + bytes /
 * link rate; constants in csrc/spg_host_rounds.cpp). spg_graph_set_shard_threshold(g, n >= 0) replaces it by "at least n
 * blankets" (0 = always; used by tests). */
/* Which driver spg_graph_marginalize uses for a single-rank NFR Tree call at the stored estimates. Default (-1): the
 * streaming driver on the HIP backend (one blanket = one item of the persistent worker kernel's queue, committed as its
 * ready word arrives; blankets the worker does not take fall back to the batch driver), the batch driver on an injected
 * backend. seed >= 0: tests — the streaming driver also runs on an injected backend, its "device" completing the
 * blankets in flight in an order drawn from the seed (0: all, oldest first). seed = -2: never stream (A/B). */
int spg_graph_set_stream_emulation(spg_graph *g, int seed);
/* per-removed-vertex diagnostics of the last marginalize call, in processing order */
int spg_graph_last_blanket_count(const spg_graph *g);
int spg_graph_last_blankets(const spg_graph *g, int32_t *root_id, int32_t *round, int32_t *status,
                            int32_t *info, double *kld, double *min_gap);

/* computeSubstituteEdge (src/compute_substitute_edge.cpp:13-96), host-side: for the online / cluster
 * replay harness, when a new edge (*from,*to) points at an already marginalised vertex. g is the FULL
 * source graph; marginalized = ids removed so far; maxid = newest vertex. On return the marginalised
 * endpoint is replaced by the nearest surviving vertex, meas (3|7) and info_upper (6|21) are filled. */
int spg_graph_substitute_edge(spg_graph *g, const int32_t *marginalized, int n_marg, int maxid,
                              int *from, int *to, double *meas, double *info_upper);

/* ---- global Kullback-Leibler divergence ------------------------------------
 * other->information() / sparseInformation() (src/graph_wrapper_g2o.cpp:351-396): the dense
 * Gauss-Newton information of the graph at its stored estimates over all vertices except the fixed one
 * (fixed_id < 0: the smallest id, which is the vertex the reference fixes and skips), id order,
 * n = pose_dim * (V - 1). Returns n; the n x n row-major matrix is written if cap >= n*n. */
int64_t spg_graph_information(spg_graph *g, int32_t fixed_id, double *out, int64_t cap);
/* The same matrix in block-CSR form at any size (GraphWrapperG2O::sparseInformation, src/graph_wrapper_g2o.cpp:382-396):
 * D x D row-major blocks; block rows and columns are the live vertices except the fixed one in ascending id order (the
 * conventions of spg_graph_information); the full symmetric pattern (both triangles), columns ascending within a row,
 * the diagonal block always present. A binary edge contributes its pair, a GLC or MULTI edge the clique of its
 * vertices, a self-loop nothing; parallel edges accumulate into one block. Block (u, v) is the transpose of block
 * (v, u) bit for bit, and the values equal those of spg_graph_information. Returns the number of blocks nnzb; the arrays
 * (row_ptr: nb + 1, col_idx: nnzb, blocks: nnzb D^2 doubles, ids: nb vertex ids, may be NULL) are written only when
 * row_ptr and col_idx are given and cap_blocks >= nnzb. blocks == NULL: the pattern only — host work, any backend.
 * Arguments are checked (SPG_EINVAL) before the backend; values need the HIP backend (SPG_ESTATE); the only size limit
 * is free device memory (SPG_ECAPACITY). */
int64_t spg_graph_sparse_information(spg_graph *g, int32_t fixed_id, int64_t *row_ptr, int32_t *col_idx, double *blocks,
                                     int64_t cap_blocks, int32_t *ids);
/* Y = H X with that matrix, which is assembled block-CSR on the device and never formed densely: X and Y hold nrhs
 * vectors of length n = D nb, one after the other. Same checks and error codes. */
int spg_graph_information_apply(spg_graph *g, int32_t fixed_id, const double *X, int nrhs, double *Y);
/* kullbackLeiblerDivergence(diff, infox, maty, InformationInformation) (src/utils.cpp:70-97):
 * kld = 0.5 * (innerprod + mahalanobis - logdetx - logdety - n), logdety = -sum log D(maty). */
typedef struct {
    double kld, innerprod, mahalanobis, logdetx, logdety;
    int64_t n;               /* variables compared: pose_dim * (kept vertices - fixed) */
    int64_t n_marginalized;  /* baseline variables marginalised out */
    double device_seconds;   /* HIP-event time of assembly + factorisations + solve */
    int32_t solver;          /* SPG_SOLVER_DENSE or SPG_SOLVER_SPARSE: what ran */
    int32_t supernodes;      /* sparse: fronts of the two factorisations' assembly trees */
    double front_bytes;      /* sparse: bytes of fronts in HBM */
    double factor_flops;     /* sparse: flops of the two factorisations */
} spg_kld_terms;
/* baseline->kullbackLeibler(other) (src/graph_wrapper_g2o.cpp:531-548): marginal of the baseline's
 * information onto other's vertices (computeIndices :472-499), estimateDifference (:550-575), then the
 * formula above. Dense on the device up to 46 k variables; beyond that (or when the context's linear solver is
 * SPG_SOLVER_SPARSE) the block-sparse multifrontal path: the baseline is factorised with its marginalised vertices
 * eliminated first, log det of the marginal from the kept supernodes, trace(maty^-1 infox) from the selected
 * inverse — the reference's dense n_g x n_g step (720 GB at 100 k poses) is never formed. other's vertices must
 * be a subset of the baseline's; both graphs must live on the same device. SPG_ENOTPD if either information
 * matrix is not PD. */
int spg_graph_kullback_leibler(spg_graph *baseline, spg_graph *other, int32_t fixed_id, spg_kld_terms *out);

/* ---- per-pose covariances from the sparse factor ---------------------------------------------------
 * GraphWrapperISAM::covariance() (src/graph_wrapper_isam.cpp:259-262) asks iSAM for covariances().marginal(nodes):
 * selected blocks of the inverse read from the sparse factor, where GraphWrapperG2O::covariance()
 * (src/graph_wrapper_g2o.cpp:368-373, spg_graph_covariance) inverts the whole matrix. Here: the graph's information
 * is factorised block-sparse over its own plan (nested dissection, no marginalised part), the selected inverse
 * (Takahashi's recurrence) runs over every supernode and the requested blocks are read from it on the device. One
 * route at every size: spg_ctx_set_linear_solver does not apply. Shared conventions: the gauge of spg_graph_covariance
 * (fixed_id < 0: the smallest id), the fixed vertex's block is zero; ids, pairs and the fixed vertex are checked
 * (SPG_EINVAL) before the backend (SPG_ESTATE without HIP); SPG_ENOTPD if an information matrix is not PD. */
typedef struct {
    double device_seconds;          /* HIP-event time: assembly + factorisation + selected inverse + extraction */
    int32_t supernodes;             /* fronts of the assembly tree(s) */
    double front_bytes;             /* bytes of fronts and of the selected inverse's Z blocks in HBM */
    double factor_flops;            /* flops of the factorisation(s) */
    double selinv_flops;            /* flops of the selected inverse's tile products (pads included) */
} spg_cov_stats;
/* The D x D marginal covariance of each listed vertex, row-major, in the order given; ids == NULL: every live vertex in
 * ascending id order (n is ignored). Returns the number of doubles needed (count * D^2); writes only when
 * out && cap >= that. */
int64_t spg_graph_marginal_covariances(spg_graph *g, int32_t fixed_id, const int32_t *ids, int n, double *out, int64_t cap,
                                       spg_cov_stats *stats);
/* For each of the n pairs (a, b) (pairs[2i], pairs[2i+1]), a != b vertices of one common live edge (binary, GLC or
 * MULTI), the 2D x 2D block [[Saa, Sab], [Sba, Sbb]] row-major. A pair without a common edge is SPG_EINVAL (arbitrary
 * pairs: spg_graph_pair_covariances). Returns n (2D)^2; writes only when out && cap >= that. */
int64_t spg_graph_joint_covariances(spg_graph *g, int32_t fixed_id, const int32_t *pairs, int n, double *out, int64_t cap,
                                    spg_cov_stats *stats);
/* Per-vertex KLD: for every live vertex of other except the fixed one, kullbackLeiblerDivergence(diff, infox, maty,
 * InformationInformation) (src/utils.cpp:70-97) with infox = Sx_ii^-1 (other's marginal), maty = Sy_ii^-1 (the
 * baseline's) and diff as in spg_graph_kullback_leibler. Preconditions and error codes of spg_graph_kullback_leibler.
 * Returns the count; writes ids (ascending) and kld when both are given and cap >= the count. */
int spg_graph_marginal_kld(spg_graph *baseline, spg_graph *other, int32_t fixed_id, int32_t *ids, double *kld, int cap,
                           spg_cov_stats *stats);

/* ---- covariance of arbitrary pose pairs and pose sets ------------------------------------------------
 * Blocks outside the fronts (two vertices without a common live edge) are columns of Sigma = H^-1 solved through the
 * fronts: Sigma[:, b] = L^-T L^-1 E_b with D right-hand sides per column vertex b, batched into panels of up to 512
 * right-hand sides, the forward sweep over the fronts on b's path to the root only and the backward sweep over the
 * paths to the requested rows only. One column serves every off-pattern partner of its vertex (greedy cover: one vertex
 * against all others is one column). Diagonal and in-pattern blocks are read from the selected inverse as the calls
 * above read them (bit for bit equal to spg_graph_marginal_covariances / _joint_covariances); the solved ones agree with
 * them to rounding. Conventions of the calls above (gauge, zero fixed block, argument errors before the backend,
 * SPG_ESTATE without HIP, SPG_ENOTPD); SPG_ECAPACITY if the panels of one batch do not fit in free HBM. */
typedef struct {
    spg_cov_stats cov;        /* as above; device_seconds covers the solves too */
    int32_t columns;          /* vertices whose D columns of Sigma were solved for */
    int32_t rhs_batches;      /* multi-RHS forward/backward sweeps run */
    double solve_flops;       /* flops of the solve tile products as executed (pads included) */
    double solve_seconds;     /* HIP-event time of the solves alone */
} spg_cov_solve_stats;
/* For each of the n pairs (a, b) (pairs[2i], pairs[2i+1]), two distinct live vertices, with or without a common edge:
 * the 2D x 2D block [[Saa, Sab], [Sba, Sbb]], row-major, the layout of spg_graph_joint_covariances. Unknown ids and
 * a == b are SPG_EINVAL. Returns n (2D)^2; writes only when out && cap >= that. */
int64_t spg_graph_pair_covariances(spg_graph *g, int32_t fixed_id, const int32_t *pairs, int n, double *out, int64_t cap,
                                   spg_cov_solve_stats *stats);
/* iSAM's covariances().marginal(list) (src/graph_wrapper_isam.cpp:259-262): the (nD) x (nD) joint covariance of n
 * distinct live vertices, in the order given, row-major. Each off-diagonal block is computed once and mirrored exactly;
 * the diagonal blocks are those of spg_graph_marginal_covariances. Unknown or duplicate ids are SPG_EINVAL; n D above 46 000 (the bound of spg_graph_covariance) is
 * SPG_ECAPACITY. Returns (nD)^2; writes only when out && cap >= that. */
int64_t spg_graph_joint_marginal_covariance(spg_graph *g, int32_t fixed_id, const int32_t *ids, int n, double *out, int64_t cap,
                                            spg_cov_solve_stats *stats);

/* ---- relative-pose covariances and loop-closure candidate scores --------------------------------------
 * How uncertain the graph is about b as seen from a. For a hypothetical binary edge a -> b with measurement z and
 * information Omega: e = its error at the stored estimates (toVectorMQT(Z^-1 Xa^-1 Xb) for SE3), J = [Ja Jb] its D x 2D
 * Jacobian at z with respect to the vertex updates spg_graph_information uses, Sigma_ab the 2D x 2D block of
 * spg_graph_pair_covariances, P = J Sigma_ab J^T the covariance of that error in the coordinates of Omega. With
 * Omega = L L^T and M = I + L^T P L (eigenvalues >= 1; Omega^-1 is never formed):
 *   chi2 = e^T Omega e
 *   d2   = (L^T e)^T M^-1 (L^T e) = e^T (P + Omega^-1)^-1 e   innovation Mahalanobis distance, chi^2 with D degrees of
 *                                                             freedom for an inlier
 *   gain = 1/2 ln det M = 1/2 (ln det H' - ln det H)          nats; H' = the information after adding the edge at the
 *                                                             same estimates
 * The relative covariance of (a, b) is P at z = the current relative pose (e = 0); P^-1 is then the information of the
 * marginal relative-pose factor between a and b, with z a record spg_graph_add_edge accepts. The pair blocks stay on the
 * device: only D^2 doubles per pair, or the scores, come back. a or b may be the fixed vertex; a pair may be listed many
 * times (several hypotheses) and costs one cross block. The graph's robust kernel is ignored and the graph is not
 * modified. Conventions and error codes of spg_graph_pair_covariances; an unknown id, a == b, a non-finite measurement
 * and an active stepwise marginalisation are SPG_EINVAL (the text names the pair) before the backend is touched. */
enum { SPG_CAND_SCORED = 0, SPG_CAND_INFO_NOT_PD = 1 };
/* n pairs of distinct live vertices. rel: n x (3|7), the current relative pose in the measurement layout of spg_graph_add_edge
 * (may be NULL). cov: n x D x D, row-major, exactly symmetric. Returns n D^2; writes only when cov && cap >= that. */
int64_t spg_graph_relative_covariances(spg_graph *g, int32_t fixed_id, const int32_t *pairs, int n, double *rel, double *cov,
                                       int64_t cap, spg_cov_solve_stats *stats);
/* n candidate binary edges. ij: n x 2. records: n x (meas + info upper triangle), the layout of spg_graph_add_edges.
 * d2, gain, chi2: n each, each may be NULL. status: n, may be NULL. 0 = scored. SPG_CAND_INFO_NOT_PD = 1: Omega not positive definite
 * or not finite; that candidate's three values are NaN and the call still succeeds. Returns n; writes when cap >= n.
 * The graph is not modified. */
int spg_graph_score_candidates(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n,
                               double *d2, double *gain, double *chi2, int32_t *status, int cap, spg_cov_solve_stats *stats);

/* ---- greedy selection of candidates by conditional information gain ------------------------------------
 * Which k of n candidate edges are jointly most informative. `gain` above scores each candidate against the graph as it
 * stands: ten hypotheses that close the same loop each show that loop's full gain. Here, with the J_i, e_i, L_i of
 * spg_graph_score_candidates at the stored estimates (which do not move during the call), Sigma in the gauge of fixed_id and
 * C_ij = J_i Sigma_(ai bi),(aj bj) J_j^T (D x D; C_ii is the P above), rounds t = 0, 1, ... run on the device:
 *   gain_i(t) = 1/2 ln det(I + L_i^T C_ii(t) L_i)          the conditional gain given the edges chosen so far
 *   i*        = argmax over the eligible candidates, ties to the lowest index
 *   M = I + L*^T C**(t) L* = G G^T,  B_i,t = C_i*(t) L* G^-T,  C_ii(t+1) = C_ii(t) - B_i,t B_i,t^T,
 *   C_ij(t) = C_ij(0) - sum_{s<t} B_i,s B_j,s^T
 * which is Sigma' = Sigma - Sigma A^T (Omega^-1 + A Sigma A^T)^-1 A Sigma restricted to candidate space (Omega^-1 is
 * never formed). The sum of the selected conditional gains is 1/2 (ln det H_final - ln det H_0), H_final the information
 * after spg_graph_add_edge of the selected candidates at the same estimates.
 * Eligible: Omega finite and positive definite (else SPG_CAND_INFO_NOT_PD) and, when max_d2 > 0, d2 <= max_d2 (else
 * SPG_CAND_GATED). d2 is that of spg_graph_score_candidates on the graph as it stands: the gate is evaluated once, before
 * round 0, and NOT re-evaluated as edges are selected. Selection stops after k rounds, when no candidate is eligible, or
 * when the best conditional gain is < min_gain.
 * The joint covariance of the m distinct non-fixed endpoints (m D x m D, each unordered pair solved once, as
 * spg_graph_joint_marginal_covariance) and a history of min(k, n) D^2 doubles per candidate stay on the device: m D above
 * 46 000, or a joint block and history beyond free HBM, are SPG_ECAPACITY before anything runs (the default method,
 * SPG_GREEDY_JOINT; spg_ctx_set_greedy_method below lifts the bound with SPG_GREEDY_LAZY). a or b may be the fixed
 * vertex, a pair may be listed many times, the graph is not modified and its robust kernel is ignored. An unknown id,
 * a == b, a non-finite measurement, an unknown fixed vertex, k < 0 and an active stepwise marginalisation are SPG_EINVAL
 * (the text names the pair) before the backend is touched; SPG_ESTATE without HIP. */
enum { SPG_CAND_GATED = 2, SPG_CAND_SELECTED = 3 };
typedef struct {
    spg_cov_solve_stats solve;   /* the covariance part; its device_seconds covers the selection too */
    int32_t rounds;              /* rounds run = candidates selected */
    int32_t endpoints;           /* m */
    double select_seconds;       /* HIP-event time of the selection alone: initial gains, the rounds, final gains */
} spg_select_stats;
/* ij, records, n: as spg_graph_score_candidates. selected, cond_gain: min(k, n) entries in order of selection, cond_gain[t]
 * = the conditional gain of selected[t] when it was chosen; entries beyond the return value are -1 / NaN. final_gain (n, may
 * be NULL): the conditional gain after the last round, NaN for selected, gated and not-PD candidates. status (n, may be
 * NULL): SPG_CAND_SCORED (eligible, not selected), _INFO_NOT_PD, _GATED or _SELECTED. A candidate whose downdated C_ii
 * rounding has made indefinite gets a NaN gain: it is never picked and stays SPG_CAND_SCORED with a NaN final_gain. The
 * free-HBM check covers the joint block and the histories and runs before anything is allocated or launched; the factor's
 * fronts are checked against what is then left (SPG_ECAPACITY as in the covariance calls). Returns the number selected; with
 * cap < min(k, n) (or selected / cond_gain NULL) returns min(k, n) and writes nothing. n = 0 or k = 0 returns 0. */
int spg_graph_select_candidates(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n, int k,
                                double min_gain, double max_d2, int32_t *selected, double *cond_gain, int cap,
                                double *final_gain, int32_t *status, spg_select_stats *stats);

/* ---- greedy edge pruning by conditional information loss ---------------------------------------------------
 * Which k of n of the graph's own binary edges cost the least information when they are removed together: the recurrence
 * above with the sign turned. A prune candidate is a live binary edge, named by its index in the order of
 * spg_graph_get_edges; its measurement z_i and information Omega_i = L_i L_i^T are read from the edge's record. With J_i
 * at z_i, Sigma the covariance of the graph WITH all its edges in the gauge of fixed_id (estimates do not move, the robust
 * kernel is ignored) and C_ij(0) = J_i Sigma_(ai bi),(aj bj) J_j^T, rounds t = 0, 1, ... run on the device:
 *   M_i(t)    = I - L_i^T C_ii(t) L_i = G G^T               eigenvalues in [0, 1]; singular exactly when removing the edge
 *                                                           makes H singular (a bridge, the last constraint of a direction)
 *   margin_i  = the smallest squared pivot of that Cholesky factorisation
 *   loss_i(t) = -1/2 ln det M_i(t) >= 0                     = 1/2 (ln det H - ln det(H - A_i^T Omega_i A_i)), nats
 *   i*        = argmin over the eligible candidates, ties to the lowest index
 *   B_i,t = C_i*(t) L* G^-T,  C_ii(t+1) = C_ii(t) + B_i,t B_i,t^T,  C_ij(t) = C_ij(0) + sum_{s<t} B_i,s B_j,s^T
 * which is Sigma' = Sigma + Sigma A^T (Omega^-1 - A Sigma A^T)^-1 A Sigma restricted to candidate space.
 * Eligible in round t (re-evaluated EVERY round: an edge becomes a bridge when its parallel path is cut): not yet pruned,
 * Omega finite and positive definite, the factorisation completes and margin >= min_margin (<= 0: the default 1e-6).
 * Margins only shrink as edges go (C_ii grows in the PSD order), so a candidate that was a bridge in some round never
 * becomes eligible again. Pruning stops after k rounds, when nothing is eligible, when the best loss is > max_loss
 * (max_loss <= 0: no limit) or when the cumulative KLD would exceed max_kld (<= 0: no limit).
 *   kld(t) = sum_{s<=t} loss_s - 1/2 sum_{s<=t} tr(L_s^T C_ss(0) L_s)
 * is the exact KLD of the pruned graph against the original at the same estimates: what spg_graph_kullback_leibler on the
 * original with the pruned graph as `other` returns, 1/2 (tr(H_p Sigma) - N + ln det H - ln det H_p), mean term 0.
 * Memory and SPG_ECAPACITY exactly as spg_graph_select_candidates (joint covariance of the distinct non-fixed endpoints,
 * min(k, n) D^2 doubles of history per candidate; spg_ctx_set_greedy_method below). An endpoint may be the fixed vertex. The graph is NOT modified: apply
 * the result with spg_graph_remove_edges. An index out of range, a non-binary edge (GLC, MULTI), an index listed twice,
 * k < 0, an unknown fixed vertex and an active stepwise marginalisation are SPG_EINVAL (the text names the candidate)
 * before the backend is touched; SPG_ESTATE without HIP. */
enum { SPG_PRUNE_KEPT = 0, SPG_PRUNE_INFO_NOT_PD = 1, SPG_PRUNE_BRIDGE = 2, SPG_PRUNE_PRUNED = 3 };
typedef struct {
    spg_cov_solve_stats solve;   /* the covariance part; its device_seconds covers the pruning too */
    int32_t rounds;              /* rounds run = edges pruned */
    int32_t endpoints;           /* m */
    double prune_seconds;        /* HIP-event time of the pruning alone: initial losses, the rounds, final values */
} spg_prune_stats;
/* pruned, cond_loss, kld: min(k, n) entries in order; pruned[t] indexes edge_idx, cond_loss[t] = its loss when it was chosen,
 * kld[t] = the cumulative KLD after round t; entries beyond the return value are -1 / NaN. Per candidate (n each, each may
 * be NULL): final_loss = the conditional loss after the last round, NaN unless the status is SPG_PRUNE_KEPT; final_margin =
 * the margin after the last round, NaN for pruned and not-PD candidates; status = SPG_PRUNE_*, _BRIDGE meaning ineligible by
 * margin after the last round. Returns the number pruned; with cap < min(k, n) (or pruned / cond_loss / kld NULL) returns
 * min(k, n) and writes nothing. n = 0 or k = 0 returns 0. */
int spg_graph_prune_candidates(spg_graph *g, int32_t fixed_id, const int32_t *edge_idx, int n, int k,
                               double max_loss, double max_kld, double min_margin,
                               int32_t *pruned, double *cond_loss, double *kld, int cap,
                               double *final_loss, double *final_margin, int32_t *status, spg_prune_stats *stats);

/* ---- outlier edges by greedy data snooping -------------------------------------------------------------------
 * Which of the graph's own binary edges are wrong: the classical normalised-residual test, each edge's leave-one-out
 * chi^2 statistic, taken greedily and re-conditioned after every rejection. A candidate is a live binary edge, named by
 * its index in the order of spg_graph_get_edges; J_i, L_i (Omega_i = L_i L_i^T), Sigma (gauge of fixed_id) and C_ij(0)
 * are those of the pruning above, and e_i(0) is the edge's error at the stored estimates. The stored estimates are TAKEN
 * AS the minimiser of the linearised problem: call spg_graph_optimize first. The gradient is not checked, and the robust
 * kernel is ignored. Rounds t = 0, 1, ... run on the device:
 *   M_i(t)    = I - L_i^T C_ii(t) L_i = G G^T            margin_i = the smallest squared pivot (as the pruning)
 *   stat_i(t) = |G^-1 L_i^T e_i(t)|^2                     = e_i^T (Omega_i^-1 - C_ii(t))^-1 e_i
 *   i*        = argmax over the eligible candidates, ties to the lowest index
 *   K = L* G^-T,  w = K^T e*(t)  (stat* = |w|^2),  B_i,t = C_i*(t) K
 *   C_ii(t+1) = C_ii(t) + B_i,t B_i,t^T,   e_i(t+1) = e_i(t) + B_i,t w
 * stat_i(t) is chi^2 with D degrees of freedom for an inlier, and equals the drop of the linearised graph's minimum chi^2
 * when the edge is left out and the rest is refitted. Eligible is re-evaluated every round exactly as the pruning does:
 * not yet flagged, Omega finite and positive definite, the factorisation completes and margin >= min_margin (<= 0: the
 * default 1e-6). Detection stops after k rounds, when nothing is eligible, or when the best statistic is < min_stat
 * (<= 0: no threshold).
 * Identities: sum_t stat*(t) = chi^2(0) - chi^2 of the linear refit without the flagged edges. redundancy_i = tr M_i(0)
 * = D - tr(L_i^T C_ii(0) L_i) lies in [0, D]; over all edges of a graph with binary edges only the redundancies sum to
 * D (E - V + 1).
 * NOT DECIDABLE: an edge at a vertex that has exactly two edges has the same statistic as that vertex's other edge (the
 * vertex absorbs either residual equally); which of the two is wrong cannot be told, and the tie goes to the lower index.
 * Memory, SPG_ECAPACITY, the greedy method, the argument errors and SPG_ESTATE exactly as spg_graph_prune_candidates
 * (the per-candidate state grows by the D doubles of e_i; the statistic takes the place of the loss). The graph is NOT modified: apply a result with
 * spg_graph_remove_edges. */
enum { SPG_OUTLIER_INLIER = 0, SPG_OUTLIER_INFO_NOT_PD = 1, SPG_OUTLIER_UNTESTABLE = 2, SPG_OUTLIER_FLAGGED = 3 };
typedef struct {
    spg_cov_solve_stats solve;   /* the covariance part; its device_seconds covers the detection too */
    int32_t rounds;              /* rounds run = edges flagged */
    int32_t endpoints;           /* m */
    double detect_seconds;       /* HIP-event time of the detection alone: initial statistics, the rounds, final values */
} spg_outlier_stats;
/* flagged, stat: min(k, n) entries in order; flagged[t] indexes edge_idx, stat[t] = its statistic when it was chosen;
 * entries beyond the return value are -1 / NaN. Per candidate (n each, each may be NULL): final_stat = the statistic after
 * the last round, NaN unless the status is SPG_OUTLIER_INLIER; final_margin = the margin after the last round, NaN for
 * flagged and not-PD candidates; redundancy as above (round 0), NaN for not-PD candidates; status = SPG_OUTLIER_*,
 * _UNTESTABLE meaning ineligible by margin after the last round (a bridge: its residual is zero by construction). Returns
 * the number flagged; with cap < min(k, n) (or flagged / stat NULL) returns min(k, n) and writes nothing. n = 0 or k = 0
 * returns 0. */
int spg_graph_detect_outliers(spg_graph *g, int32_t fixed_id, const int32_t *edge_idx, int n, int k,
                              double min_stat, double min_margin,
                              int32_t *flagged, double *stat, int cap,
                              double *final_stat, double *final_margin, double *redundancy, int32_t *status,
                              spg_outlier_stats *stats);
/* ---- how the greedy calls above get at Sigma ------------------------------------------------------------
 * SPG_GREEDY_JOINT (default): the m D x m D joint block described above, and its 46 000 bound.
 * SPG_GREEDY_LAZY: no joint block, and no bound on m D. Round 0 comes from one 2D x 2D block per distinct ordered endpoint
 *   pair (the blocks of spg_graph_relative_covariances: every prune candidate is an edge, so its block is read from the
 *   selected inverse without a column solve). Each round then solves, on the factor, the D columns of Sigma at the two
 *   endpoints of the candidate it chose, in one 64-wide right-hand-side panel, and keeps them in a column cache on the
 *   device: one strip Sigma[S, v] (m D x D) per cached vertex. Columns belong to the original Sigma and never go stale.
 *   The rest of the panel is filled with the endpoint columns of the next-best candidates. The selected inverse overwrites
 *   the factor, so a lazy call factorises a second time after round 0 (`refactorised`). What must fit in free HBM (1 GB
 *   kept free), else SPG_ECAPACITY with the sizes in the text: the pair blocks, the histories, one panel workspace and at
 *   least two strips; the cache takes what is left, at most m strips and at most what min(k, n) rounds can fill. Results are those of JOINT within rounding: the same
 *   recurrence on blocks that come from column solves instead of the joint block's mix of both.
 * SPG_GREEDY_AUTO: JOINT whenever JOINT would not return SPG_ECAPACITY (m D <= 46 000 and joint block + histories
 *   within free HBM), else LAZY. A capacity rule only.
 * lookahead: candidates whose endpoint columns one panel may hold, the chosen one included. 0 = a full panel, 64 / 2D
 *   (5 for SE3, 10 for SE2); 1 = the chosen candidate only; larger values are clamped. lookahead < 0 or an unknown method
 *   is SPG_EINVAL. Signatures, eligibility, gate, stop rules, tie order, statuses and the kld definition of the two calls
 *   are the same in every mode. */
enum { SPG_GREEDY_JOINT = 0, SPG_GREEDY_LAZY = 1, SPG_GREEDY_AUTO = 2 };
int spg_ctx_set_greedy_method(spg_ctx *ctx, int method, int lookahead);
typedef struct {
    int32_t method, lookahead;       /* the method used (JOINT or LAZY) and, for LAZY, the candidates per panel (else 0) */
    int32_t rounds, refactorised;    /* rounds run; 1 when the factor was rebuilt after the selected inverse */
    int64_t column_vertices;         /* vertices whose columns were solved during the rounds, speculative ones included */
    int64_t column_hits;             /* endpoint columns of a chosen candidate that were already cached */
    int32_t rhs_batches, evictions;  /* panels swept during the rounds; strips given up for a needed column */
    double round_solve_seconds;      /* HIP-event time of the per-round sweeps */
    double cache_bytes;              /* size of the column cache */
} spg_greedy_stats;
/* of the context's last spg_graph_select_candidates / _prune_candidates / _detect_outliers call that reached the device (all zero before) */
int spg_ctx_greedy_stats(spg_ctx *ctx, spg_greedy_stats *out);

/* ---- joint compatibility of candidates ---------------------------------------------------------------------
 * Which of n candidate edges agree with each other. The gate of the calls above tests each candidate alone against the
 * graph; where drift makes P = J Sigma J^T large against Omega^-1 that test is weak, and a group of aliased closures with a
 * common wrong offset passes it. Here, with J_i = [Ja Jb], e_i and Omega_i = L_i L_i^T of spg_graph_score_candidates at the
 * stored estimates and Sigma in the gauge of fixed_id (zero blocks stand for the fixed vertex; Omega^-1 is never formed):
 *   U_i  = L_i^T J_i (D x 2D),   w_i = L_i^T e_i,   M_ij = delta_ij I + U_i Sigma_(ai bi),(aj bj) U_j^T (D x D)
 *   d2(S) = w_S^T (M_SS)^-1 w_S = e_S^T (blockdiag Omega^-1 + A_S Sigma A_S^T)^-1 e_S      chi^2 with |S| D degrees of
 *                                                       freedom when every member of S is an inlier; M_SS >= I always
 * Eligible: as the selection. Omega finite and positive definite (else SPG_CAND_INFO_NOT_PD) and, when max_d2 > 0,
 * d2_i = d2({i}) <= max_d2 (else SPG_CAND_GATED); d2_i is the d2 of spg_graph_score_candidates.
 * Stage 1, the pair test. For every unordered eligible pair i < j, d2_ij = d2({i, j}) by block elimination with i first,
 * D x D work only: d2_ij = d2_i + |G^-1 (w_j - M_ji M_ii^-1 w_i)|^2 with G G^T = M_jj - M_ji M_ii^-1 M_ij. The pair is
 * consistent iff d2_ij <= pair_max_d2; a d2_ij that is not finite is inconsistent. Each unordered pair is computed once and
 * both adjacency bits come from that one comparison: the consistency graph is exactly symmetric. It lives on the device as
 * n rows of ceil(n / 64) 64-bit words (bit j of row i), the diagonal clear, the rows of ineligible candidates empty.
 * Stage 2, the largest consistent set, a deterministic integer heuristic. For every eligible seed s: R = (s), P = N(s);
 * while P is not empty take v = argmax over u in P of |N(u) & P| (ties: the lowest index), append v to R and set
 * P = P & N(v). The answer is the longest R (ties: the lowest seed), its members in the order they were added. Every R is
 * a clique of the consistency graph that no vertex extends; it is not guaranteed to be a maximum clique.
 * Stage 3, the sequential joint gate. The members of that set are walked in ascending d2_i (ties: the lowest index),
 * S = {} and D2 = 0 at the start. For member i the left-looking block-Cholesky step
 *   G_iS = M_iS G_SS^-T,   G_ii G_ii^T = M_ii - G_iS G_iS^T,   y_i = G_ii^-1 (w_i - G_iS y_S),   t = D2 + |y_i|^2 = d2(S + {i})
 * is formed, and i is accepted iff joint_max_d2 == NULL or t <= joint_max_d2[|S|] (a t that is not finite is a rejection).
 * Accepted: the block row is appended, D2 = t, SPG_CAND_SELECTED. Rejected: the row is dropped, SPG_CAND_INCOMPATIBLE. The
 * walk stops after k acceptances; members never examined, and eligible candidates outside the set, stay SPG_CAND_SCORED.
 * The call always takes the joint block of the m distinct non-fixed endpoints (m D <= 46 000, as SPG_GREEDY_JOINT;
 * spg_ctx_set_greedy_method is ignored here). SPG_ECAPACITY, before anything is allocated: n above 16 384, m D above
 * 46 000, or the joint block, the consistency graph, the stage-3 workspace ((min(k, n) D)^2 doubles of factor plus the
 * rows) and a requested pair_d2 together beyond free HBM (1 GB kept free). Argument errors as spg_graph_select_candidates
 * (the text names the pair), and pair_max_d2 <= 0, a clique_cap below n with clique given, a pair_cap below n^2 with pair_d2
 * given: SPG_EINVAL before the backend is touched; SPG_ESTATE without HIP. The graph is not modified and its robust kernel
 * is ignored. */
enum { SPG_CAND_INCOMPATIBLE = 4 };
typedef struct {
    spg_cov_solve_stats solve;   /* the covariance part; its device_seconds covers the three stages too */
    int32_t endpoints;           /* m */
    int32_t eligible;            /* candidates that took part in the pair test */
    int64_t consistent_pairs;    /* edges of the consistency graph */
    int32_t clique_size, seed;   /* stage 2: the size of the set and the seed that reached it (-1: nobody eligible) */
    double pair_seconds;         /* HIP-event times: the per-candidate terms and stage 1, */
    double clique_seconds;       /* stage 2, */
    double verify_seconds;       /* stage 3 */
} spg_compat_stats;
/* ij, records, n, max_d2: as spg_graph_select_candidates. joint_max_d2: min(k, n) thresholds (entry p gates the set of p + 1)
 * or NULL. compatible, joint_d2: min(k, n) entries, the accepted candidates in order and d2(S) after each; entries beyond
 * the return value are -1 / NaN. clique (clique_cap >= n entries, may be NULL): the stage-2 set in order of construction,
 * -1 beyond stats->clique_size. d2, degree, status: n each, each may be NULL; degree = the candidate's row sum of the
 * consistency graph. pair_d2 (pair_cap >= n^2, may be NULL): n x n, exactly symmetric, the diagonal = d2_i, NaN in the rows
 * and columns of ineligible candidates. Returns the number accepted; with cap < min(k, n) (or compatible / joint_d2 NULL)
 * returns min(k, n) and writes nothing. n = 0 or k = 0 returns 0. */
int spg_graph_compatible_candidates(spg_graph *g, int32_t fixed_id, const int32_t *ij, const double *records, int n, int k,
                                    double max_d2, double pair_max_d2, const double *joint_max_d2,
                                    int32_t *compatible, double *joint_d2, int cap,
                                    int32_t *clique, int clique_cap,
                                    double *d2, int32_t *degree, int32_t *status,
                                    double *pair_d2, int64_t pair_cap,
                                    spg_compat_stats *stats);
/* Stage 2 alone on a caller's consistency graph, for a metric of the caller's own (inter-robot closures with no common
 * graph). adj: n rows of ceil(n / 64) words, bit j of row i. SPG_EINVAL if adj is not symmetric, has a diagonal bit set or
 * has bits at or beyond n; SPG_ECAPACITY for n above 16 384; SPG_ESTATE without HIP. Returns the size of the set; n = 0
 * returns 0. clique (may be NULL): the members in order of construction, written when cap >= the size. seed (may be NULL):
 * the seed that reached it. */
int spg_ctx_max_clique(spg_ctx *ctx, int n, const uint64_t *adj, int32_t *clique, int cap, int32_t *seed);

/* ---- proposal of candidates by proximity and range -----------------------------------------------------------
 * Where the pairs ij of the calls above come from: which old poses the current poses might see. Two stages, both on the
 * device, at the stored estimates; the graph is not modified and its robust kernel is ignored.
 * Stage A, the geometric search. p_v = the translation of vertex v (xy / xyz). Two distinct live vertices, written with
 * id_a < id_b, QUALIFY iff
 *   1. dist = |p_a - p_b|_2 <= search_radius (search_radius > 0 and finite);
 *   2. max_angle <= 0, or the rotation angle of X_a^-1 X_b is <= max_angle (SE2: |wrap(theta_b - theta_a)|, SE3:
 *      2 atan2(|vec|, |w|) of q_a^-1 q_b);
 *   3. min_id_gap <= 1, or id_b - id_a >= min_id_gap (the convention of spg_graph_set_robust_kernel);
 *   4. no live edge of any kind (binary, GLC, MULTI) has both a and b among its vertices;
 *   5. queries == NULL (every live vertex is a query), or a or b is one of the n_queries distinct live ids listed.
 * The per-vertex cap max_per_vertex = m (0: none; above 32: SPG_EINVAL): for every query v its qualifying partners are
 * ordered by (dist, partner id) ascending and tau_v is the m-th entry, +inf with fewer than m. A qualifying pair is KEPT
 * iff a is a query and (dist, id_b) <= tau_a, or b is a query and (dist, id_a) <= tau_b: the symmetrised m-nearest-
 * neighbour graph, every pair once. The kept pairs are reported in ascending (id_a, id_b) order with dist and angle (the
 * angle also when max_angle <= 0).
 * The search is a uniform grid with cell edge search_radius: cell coordinate floor(p / search_radius) per axis, 21 signed
 * bits per axis in one 64-bit key, the cells in an open-addressing hash table of 2^ceil(log2(2 n_live)) slots. A pose that is
 * not finite is SPG_EINVAL, one whose cell coordinate does not fit SPG_ECAPACITY, both with the vertex id in the text and
 * before anything is searched. Each query tests the poses of its 3^dim cells only (stats.pairs_tested). The result does
 * not depend on the order of the device's atomics: two calls return the same bits. The environment variable
 * SPG_PROPOSE_TABLE_BITS=b (diagnostic) forces a table of 2^b slots: SPG_ECAPACITY when the occupied cells exceed it.
 * Stage B, the range gate under uncertainty, runs when range > 0 (range > search_radius: SPG_EINVAL), AFTER the cap
 * of stage A, which so bounds the covariance columns solved. For every kept pair P = J Sigma_ab J^T at z = the current
 * relative pose, exactly what spg_graph_relative_covariances computes and at its cost (one column per distinct vertex of
 * the greedy cover; stats.solve), stays on the device, and with rho = |t_z|, u = R_z^T t_z / rho,
 *   sigma^2 = u^T P_tt u,   zscore = (rho - range) / sigma    (sigma = 0: -inf when rho <= range, else +inf)
 * the pair passes iff zscore <= z_max, or rho <= range (then zscore <= 0, and the pair passes whatever sigma and z_max
 * are). Failing pairs are dropped, the order stays. fixed_id: the gauge convention of the covariance calls; a or b may be the fixed vertex. At 100 000 poses the
 * intended use of stage B is a query list of a few recent poses: one query against all its neighbours is one column.
 * Errors, before the backend is touched and with the offending id in the text (SPG_EINVAL): search_radius, z_max = NaN,
 * max_per_vertex, range, an unknown or repeated query id, an unknown fixed vertex, an active stepwise marginalisation.
 * SPG_ESTATE without HIP. A graph with fewer than two live vertices, an empty query list or no kept pair returns 0. */
typedef struct {
    spg_cov_solve_stats solve;    /* stage B (all zero when range <= 0) */
    int32_t n_cells;              /* occupied cells */
    int32_t max_cell_population;
    int64_t table_slots;
    int64_t pairs_tested;         /* ordered (query, partner) distance evaluations of pass 1 */
    int64_t n_qualifying;         /* pairs under rules 1 to 5, before the cap */
    int64_t n_kept;               /* after the cap */
    int64_t n_gated;              /* after stage B (= n_kept when range <= 0) */
    double device_seconds;        /* HIP-event time of stage A alone */
} spg_propose_stats;
/* ij: 2 per pair; dist, angle: 1 per pair; sigma, zscore (may be NULL; written when range > 0): 1 per pair. Returns the
 * number of pairs; writes only when ij, dist and angle are given and cap >= that number. With range <= 0 a call with
 * cap = 0 costs the search without the fill; with range > 0 the count needs the whole of stage B. */
int64_t spg_graph_propose_candidates(spg_graph *g, int32_t fixed_id, double search_radius, double max_angle, int32_t min_id_gap,
                                     int32_t max_per_vertex, const int32_t *queries, int n_queries, double range, double z_max,
                                     int32_t *ij, double *dist, double *angle, double *sigma, double *zscore, int64_t cap,
                                     spg_propose_stats *stats);

/* ---- selection of the vertices to remove by spatial redundancy ----------------------------------------------
 * Which vertices should go: one pose is kept per neighbourhood, so that a place visited a hundred times costs what it
 * costs when visited once. On the device, at the stored estimates; the graph is not modified and its robust kernel is
 * ignored. Two distinct live vertices are REDUNDANT iff
 *   1. |p_a - p_b|_2 <= radius (radius > 0 and finite): rule 1 of spg_graph_propose_candidates, the same arithmetic;
 *   2. max_angle <= 0, or the rotation angle of X_a^-1 X_b is <= max_angle: rule 2, asked with a the lower id.
 * There is no adjacency rule, no id-gap rule and no query list. The live vertices are put in a total ORDER: the n_keep
 * vertices of `keep` first; then the others, by (priority descending, id ascending) when priority is given (one double per
 * live vertex in ascending-id order; a NaN is SPG_EINVAL with the id in the text), and with priority == NULL by
 * (mix64((uint64)(uint32)id), id) ascending, mix64 the splitmix64 finaliser (x ^= x >> 30, x *= 0xbf58476d1ce4e5b9,
 * x ^= x >> 27, x *= 0x94d049bb133111eb, x ^= x >> 31) with all 64 bits kept.
 * The KEPT set K is the lexicographically first maximal independent set in that order: K starts as the keep list (forced
 * vertices are kept even when they are redundant with each other); every other vertex, taken in order, joins K iff no
 * member of K is redundant with it. Everything not in K is REMOVED, and the REPRESENTATIVE of a removed vertex is the kept
 * vertex redundant with it of smallest (dist, id). So every removed vertex has a kept vertex within radius, no two unforced
 * kept vertices are redundant, and a second call on the resulting graph removes nothing.
 * The grid, its table, SPG_PROPOSE_TABLE_BITS and the refusal of poses (not finite: SPG_EINVAL; a cell coordinate that does
 * not fit: SPG_ECAPACITY; both with the vertex id) are those of spg_graph_propose_candidates with cell edge = radius.
 * The decision runs in rounds, one kernel launch each, until every vertex is decided; the result does not depend on the
 * order of the device's atomics: two calls return the same bits. stats.rounds and stats.pairs_tested may differ between
 * calls. An order that follows the trajectory (priority by id) makes long chains of dependent decisions and so many rounds;
 * the hashed default keeps them short.
 * Errors, before the backend is touched and with the offending id in the text (SPG_EINVAL): radius not finite or <= 0,
 * max_angle = NaN, an unknown or repeated keep id, a NaN priority, an active stepwise marginalisation. SPG_ESTATE without
 * HIP. Zero or one live vertex returns 0. */
typedef struct {
    int32_t n_cells, max_cell_population; int64_t table_slots;   /* as spg_propose_stats */
    int32_t n_live, n_forced, n_kept, n_removed;
    int32_t rounds;               /* launches of the decision kernel; diagnostic, may differ between calls */
    int64_t pairs_tested;         /* distance evaluations of the decision kernel; diagnostic, may differ between calls */
    double device_seconds;        /* HIP-event time from the grid to the output, the host's reads between the rounds included */
} spg_removal_stats;
/* removed (ascending ids), representative, rep_dist: 1 per removed vertex. Returns the number of removed vertices; writes
 * only when the three are given and cap >= that number. The ids go unchanged into spg_graph_marginalize. */
int64_t spg_graph_select_removals(spg_graph *g, double radius, double max_angle, const int32_t *keep, int n_keep,
                                  const double *priority, int32_t *removed, int32_t *representative, double *rep_dist,
                                  int64_t cap, spg_removal_stats *stats);

/* Removes n live edges of any kind, named by their indices in the order of spg_graph_get_edges (the edge order is
 * canonicalised first, as spg_graph_get_edges does). Survivors keep their relative order. Bridges may be removed: a
 * disconnected graph later shows as SPG_ENOTPD. An index out of range or listed twice and an active stepwise
 * marginalisation are SPG_EINVAL; nothing is changed on error. Host only. */
int spg_graph_remove_edges(spg_graph *g, const int32_t *edge_idx, int n);

/* ---- optimize() -------------------------------------------------------------
 * GraphWrapperG2O::optimize() (src/graph_wrapper_g2o.cpp:250-269): one vertex fixed (fixed_id < 0: the
 * smallest id), g2o's Levenberg-Marquardt for up to `iterations` iterations (the reference uses 50),
 * plain least squares unless the graph has a robust kernel (spg_graph_set_robust_kernel below). On the device (Hessian assembly, Cholesky of H + lambda I, triangular solves, pose updates,
 * chi2): dense (blocked fp64-MFMA Cholesky) up to 12 k scalar variables, block-sparse multifrontal (nested
 * dissection on the host, fronts on the matrix cores: CHOLMOD's role) beyond — see spg_ctx_set_linear_solver.
 * The estimates of the graph are updated in place. */
enum { SPG_SOLVER_AUTO = 0, SPG_SOLVER_DENSE = 1, SPG_SOLVER_SPARSE = 2, SPG_SOLVER_PCG = 3 };
/* Which factorisation spg_graph_optimize / _optimize_fixed / _kullback_leibler of graphs of this context use.
 * AUTO (default): by size. DENSE beyond its capacity (32 k / 46 k variables) returns SPG_ECAPACITY. The covariance
 * blocks (spg_graph_marginal_covariances / _joint_covariances / _marginal_kld) are always block-sparse.
 * PCG (g2o's third solver family; AUTO never chooses it): spg_graph_optimize / _optimize_fixed solve each LM trial
 * (H + lambda I) x = b by block-Jacobi preconditioned conjugate gradients on the block-CSR matrix of
 * spg_graph_sparse_information, without a factorisation. A solve that does not reach the tolerance is not an error: its
 * iterate is an inexact LM step, guarded by LM's gain test and counted in spg_pcg_stats. The KLD calls need log
 * determinants and the covariance calls the factor: both treat PCG as AUTO. */
int spg_ctx_set_linear_solver(spg_ctx *ctx, int solver);
/* PCG parameters of the context: stop at ||r|| <= rel_tol ||b|| or after max_iter iterations. <= 0: the defaults,
 * rel_tol = 1e-10 and max_iter = min(n, 20000) (g2o iterates up to n). */
int spg_ctx_set_pcg(spg_ctx *ctx, double rel_tol, int max_iter);
/* Factor-descent parameters of the context (SPG_FLAG_NFR_FACTOR_DESCENT): stop after the first cycle whose KLD decrease
 * is <= rel_tol * max(1, |KLD|), or after max_cycles cycles. A value <= 0 selects the default, rel_tol = 1e-12 and
 * max_cycles = 2000 — except rel_tol == 0 together with max_cycles > 0, which runs exactly max_cycles cycles.
 * max_cycles > 32767 (the width of the count in info >> 8) is SPG_EINVAL. Contexts of other backends accept and ignore it. */
int spg_ctx_set_factor_descent(spg_ctx *ctx, double rel_tol, int max_cycles);
typedef struct {
    int32_t solves, unconverged;         /* linear systems solved by PCG; those that stopped at max_iter */
    int64_t iterations;                  /* CG iterations over all solves */
    double last_rel_residual;            /* ||r|| / ||b|| of the recurrence at the end of the last solve */
    double solve_seconds;                /* host time of the solves (they end with a synchronisation) */
} spg_pcg_stats;
/* of the last spg_graph_optimize / _optimize_fixed call of the context (all zero if it did not run PCG) */
int spg_ctx_pcg_stats(spg_ctx *ctx, spg_pcg_stats *out);
typedef struct {
    int32_t iterations, trials;          /* LM iterations run; linear systems solved */
    double chi2_initial, chi2_final, lambda_final;
    int64_t n;                           /* scalar variables */
    double device_seconds;
    int32_t solver;                      /* SPG_SOLVER_DENSE, SPG_SOLVER_SPARSE or SPG_SOLVER_PCG: what ran */
    int32_t supernodes;                  /* sparse: fronts of the assembly tree */
    double front_bytes;                  /* sparse: bytes of fronts in HBM */
    double factor_flops;                 /* sparse: flops of one factorisation */
} spg_optimize_stats;
int spg_graph_optimize(spg_graph *g, int iterations, int32_t fixed_id, spg_optimize_stats *out);
/* Symbolic phase of the block-sparse solver on its own (host only; inspection and CPU tests): nested-dissection
 * elimination order and assembly tree of a block graph given as symmetric CSR adjacency. is_marg (may be NULL): blocks
 * to eliminate first (the global KLD's marginalised vertices). leaf <= 0: default leaf size. Every output array may be
 * NULL; rows / rel are written only if rows_cap >= info->n_rows. perm[position] = block; supernode s owns positions
 * [sn_first[s], sn_first[s+1]); rows[sn_rowptr[s] ..) = its boundary positions (ascending); rel = scalar offset of each
 * boundary block inside the PARENT's front ([pivot columns padded to 64 | boundary rows]). */
typedef struct {
    int32_t n_supernodes, n_marg_supernodes, n_levels, pad_;
    int64_t n_rows;
    double front_bytes, flops;
} spg_sparse_plan_info;
int spg_sparse_plan(int n_blocks, const int32_t *adj_ptr, const int32_t *adj, int pose_dim, const uint8_t *is_marg, int leaf,
                    spg_sparse_plan_info *info, int32_t *perm, int32_t *sn_first, int32_t *sn_parent, int32_t *sn_level,
                    int32_t *sn_rowptr, int32_t *rows, int32_t *rel, int64_t rows_cap);
/* The same with a set of vertices held fixed at their current estimates — the inner step of
 * GraphWrapperG2O::chi2(other) (src/graph_wrapper_g2o.cpp:503-529): fix other's vertices at other's
 * estimates, optimise the rest, read chi2. n_fixed may cover every vertex (chi2 is evaluated, nothing moves). */
int spg_graph_optimize_fixed(spg_graph *g, int iterations, const int32_t *fixed_ids, int n_fixed, spg_optimize_stats *out);
/* _so->chi2(): sum of e^T Omega e over all edges at the current estimates (src/graph_wrapper_g2o.cpp:501,519) */
int spg_graph_chi2(spg_graph *g, double *chi2);

/* ---- initialize(): initial pose estimates from the measurements ------------------------------
 * optimize() starts from the stored estimates; this call produces them. The fixed vertex (fixed_id < 0: the smallest
 * live id) keeps its stored pose, which defines the gauge; every other live vertex's estimate is overwritten, on the
 * host and on the device, the way optimize() leaves them (SE3 quaternions unit length with w >= 0, SE2 angles in
 * (-pi, pi]). The result is a function of the measurements, the informations and the fixed pose alone: the stored
 * estimates of the other vertices are never read. Only binary pose-pose edges enter (parallel ones all do); GLC edges,
 * MULTI edges and self-loops are ignored and counted; the robust kernel is ignored.
 *
 * SPG_INIT_SPANNING_TREE (host, any backend) — g2o's computeInitialGuess with unit edge costs: breadth-first search from
 * the fixed vertex over the binary edges. The parent of a vertex is its neighbour in the previous level with the
 * smallest id; among parallel edges to it the one that comes first in the order of spg_graph_get_edges (the edge order
 * is canonicalised first, as there). Along the edge T_child = T_parent Z, against it T_child = T_parent Z^-1.
 *
 * SPG_INIT_CHORDAL (device; SPG_ESTATE without the HIP backend) — chordal relaxation (Carlone et al. 2015, GTSAM's
 * InitializePose3) with scalar weights. Edge e = (a, b), Z_e = T_a^-1 T_b = (R_ab, t_ab), information Omega_e with the
 * translation block first. Weights: kappa_e = Omega_theta_theta (SE2) or trace(Omega[3:6,3:6]) / 3 (SE3);
 * tau_e = trace(Omega_tt) / 2 (SE2) or / 3 (SE3). An edge with a weight that is not finite and > 0 is SPG_EINVAL.
 *   1. rotations: SE3 unknowns M_i = R_i^T, minimise sum kappa_e ||M_b - R_ab^T M_a||_F^2 with M_f fixed (three
 *      independent columns); SE2 unknowns m_i = (cos theta_i, sin theta_i), minimise sum kappa_e ||m_b - Rot(theta_ab) m_a||^2.
 *      Normal equations over the free vertices: diagonal blocks (sum kappa_e) I, block (b, a) -= kappa_e R_ab^T, block
 *      (a, b) -= kappa_e R_ab, the fixed vertex's terms on the right-hand side.
 *   2. projection: SE3 R_i^T = U diag(1, 1, det(U V^T)) V^T of M_i = U S V^T; SE2 theta_i = atan2(m_1, m_0). A vertex is
 *      degenerate when ||m_i|| < 1e-6 (SE2) or the second-largest singular value of M_i is below 1e-6 (SE3): it takes
 *      the orientation of the spanning tree above and is counted. (With one fixed vertex and rotation measurements that
 *      disagree around cycles, the relaxed blocks shrink with the distance from the fixed vertex: on graphs hundreds of
 *      loops deep with large rotation noise most vertices can end below this threshold. Read `degenerate`.)
 *   3. translations: minimise sum tau_e ||t_b - t_a - R_a t_ab||^2 with t_f fixed and the rotations of step 2 — the
 *      tau-weighted graph Laplacian (x) I.
 * Both systems are factorised by the block-sparse multifrontal Cholesky over one nested-dissection plan with 3 x 3
 * blocks (SE2 is embedded: Rz blocks, zero third component). spg_ctx_set_linear_solver does not apply: there is no
 * dense and no PCG route, SPG_SOLVER_PCG and every other setting behave as AUTO, as for the covariance calls. The only
 * size limit is free device memory (SPG_ECAPACITY). A failed factorisation is SPG_ENOTPD (it cannot occur on a
 * connected graph with positive weights).
 *
 * Errors, all found before anything is computed, and the graph is unchanged after any error: SPG_EINVAL for an unknown
 * method, an unknown fixed_id, an active stepwise marginalisation, a live vertex that no chain of binary edges joins to
 * the fixed one (the message names the smallest such id), a bad weight (chordal). A graph that holds only the fixed
 * vertex is a successful no-op. */
enum { SPG_INIT_SPANNING_TREE = 0, SPG_INIT_CHORDAL = 1 };
typedef struct {
    int32_t method;            /* what ran */
    int32_t n_vertices;        /* live vertices, the fixed one included */
    int32_t edges_used;        /* binary edges that entered (self-loops excluded) */
    int32_t edges_ignored;     /* GLC, MULTI and self-loop edges */
    int32_t tree_depth;        /* deepest BFS level of the spanning tree */
    int32_t degenerate;        /* chordal: vertices whose relaxed rotation could not be projected */
    double chi2_before, chi2_after;   /* spg_graph_chi2 before / after; NaN on a backend without HIP */
    double device_seconds;     /* HIP-event time of assembly + factorisations + solves + projection (0 for the tree) */
    int32_t supernodes; double front_bytes, factor_flops;   /* as in spg_optimize_stats */
} spg_init_stats;
int spg_graph_initialize(spg_graph *g, int method, int32_t fixed_id, spg_init_stats *out /* may be NULL */);

/* ---- robust kernels for optimize() -----------------------------------------------------------
 * g2o's OptimizableGraph::Edge::setRobustKernel in its IRLS form, the second-order term left out as g2o leaves it out.
 * For a binary pose-pose edge with s = e^T Omega e the kernel supplies rho(s) and the weight w = d rho / d s:
 *   cost = sum rho(s_e),   H = sum w_e J_e^T Omega_e J_e,   b = -sum w_e J_e^T Omega_e e_e.
 * With width delta > 0:
 *   SPG_ROBUST_HUBER          rho = s if s <= delta^2, else 2 delta sqrt(s) - delta^2;   w = 1, else delta / sqrt(s)
 *   SPG_ROBUST_CAUCHY         rho = delta^2 log1p(s / delta^2);                          w = 1 / (1 + s / delta^2)
 *   SPG_ROBUST_GEMAN_MCCLURE  rho = delta^2 s / (delta^2 + s);                           w = (delta^2 / (delta^2 + s))^2
 *   SPG_ROBUST_DCS (Phi = delta)  rho = c^2 s + Phi (1 - c)^2, c = min(1, 2 Phi / (Phi + s));   w = c^2
 * (DCS: w is the derivative with the switch variable c held — dynamic covariance scaling's definition and g2o's weight;
 * with c substituted rho equals Phi for every s > Phi.)
 * The kernel applies to the binary edges whose two vertex ids differ by at least min_id_gap (1: every binary edge; 2:
 * consecutive-id odometry edges are left alone; values <= 0 are treated as 1). GLC edges, MULTI edges and self-loops
 * always keep w = 1 and rho = s.
 * The setting belongs to the graph; spg_graph_clone_portion copies it, the .g2o writer does not serialise it.
 * Honoured by spg_graph_optimize and spg_graph_optimize_fixed on all three solvers: with a kernel set, chi2_initial and
 * chi2_final of spg_optimize_stats are sum rho, and LM's gain test uses sum rho. NOT honoured — plain least squares
 * whatever the setting — by spg_graph_chi2, spg_graph_information, _sparse_information, _information_apply,
 * _covariance and the covariance-block calls, both KLD calls and everything under marginalisation.
 * Usage: optimise robustly, then clear the kernel (or sparsify, which never sees it) before optimising the sparsified
 * graph: the new NFR edges are binary and would otherwise be down-weighted like measurements. */
enum { SPG_ROBUST_NONE = 0, SPG_ROBUST_HUBER = 1, SPG_ROBUST_CAUCHY = 2, SPG_ROBUST_GEMAN_MCCLURE = 3, SPG_ROBUST_DCS = 4 };
/* Host only, any backend. SPG_EINVAL: unknown kind; delta not finite and > 0 with kind != NONE (NONE ignores delta);
 * a stepwise marginalisation is active. */
int spg_graph_set_robust_kernel(spg_graph *g, int kind, double delta, int min_id_gap);
int spg_graph_get_robust_kernel(const spg_graph *g, int *kind, double *delta, int *min_id_gap);
/* Per live edge at the stored estimates, in the order of spg_graph_get_edges (the edge order is canonicalised first, as
 * there): chi2[e] = the plain s, for n-ary edges too; rho[e] and weight[e] follow the graph's kernel (s and 1 without
 * one, and for the edges it does not apply to). Returns the number of live edges; the arrays (each may be NULL) are
 * written when cap >= that count. Values need the HIP backend (SPG_ESTATE). */
int spg_graph_edge_chi2(spg_graph *g, double *chi2, double *rho, double *weight, int cap);

/* ---- round-stepping form of the same call, for multi-GPU sharding ---------------------------
 * All ranks hold a replica and run the same deterministic scheduler; rank r computes its slice of
 * each round's blankets; the caller exchanges the round's output region of the arena between
 * ranks (one all-gather over RCCL/xGMI) between compute and commit. */
typedef struct {
    int32_t n_blankets;       /* blankets scheduled in this round (all ranks) */
    int32_t my_first, my_count; /* this rank's slice */
    int64_t region_off;       /* arena offset (doubles) of the round's output region */
    int64_t chunk_len;        /* doubles per rank chunk; region = nranks * chunk_len, rank r owns chunk r */
    int32_t exchange;         /* 1: blankets are sharded, the caller must all-gather the region before commit;
                                 0: the round is small (latency-bound), every rank computes all of it redundantly
                                    (bit-identical: no atomics, fixed reduction orders) and nothing is exchanged */
    int32_t pad_;
} spg_round_info;
int spg_graph_marginalize_begin(spg_graph *g, const int32_t *which, int n, const spg_options *opts,
                                int rank, int nranks);
/* n >= 0: rounds with fewer blankets than n are computed redundantly on every rank instead of being sharded +
 * exchanged (0 = always shard); n < 0 (default): the cost model described at spg_graph_marginalize_ranks */
int spg_graph_set_shard_threshold(spg_graph *g, int min_blankets);
/* returns 1 if a round was prepared (info filled), 0 when the removal list is exhausted */
int spg_graph_round_prepare(spg_graph *g, spg_round_info *info);
int spg_graph_round_compute(spg_graph *g);   /* asynchronous on the context stream */
int spg_graph_round_commit(spg_graph *g);    /* waits, reads back the region, applies the graph update */
int spg_graph_marginalize_end(spg_graph *g, spg_marg_stats *stats);
/* device (or, for an injected backend, host) address of the arena and its capacity in doubles;
 * the arena may be re-allocated by add_* calls but never between begin and end */
void *spg_graph_arena(spg_graph *g, int64_t *capacity);
/* reserve arena capacity up front (doubles) so the address stays fixed. Also sizes and touches the host-side buffers a
 * marginalisation writes (the host mirror of the arena, the edge / log containers, the scheduler's scratch): a first touch
 * inside the call is a page fault in the commit path — measured as 55 ms instead of 25 ms per 100 k-pose marginalisation on
 * graphs whose mirror had never been touched. Call it once after loading a graph that will be sparsified (3x the loaded
 * size covers sparsity 2). */
int spg_graph_reserve(spg_graph *g, int64_t arena_doubles);

/* ---- compute backend ------------------------------------------------------------------------
 * The device side of a round, as the product's HIP backend implements it and as a test may inject
 * it (spg_ctx_create_injected): tests/ use this to run the host scheduler and the multi-rank
 * exchange on CPU-only machines with oracle/libspg_ref.so as the arithmetic. The product never
 * injects anything: spg_ctx_create always binds the HIP backend and fails without a device. */
typedef struct {
    int32_t vert_begin, n_vert, n_remove; /* into vert_pose_off[] */
    int32_t edge_begin, n_edge;           /* into edge refs */
    int32_t n_new_max;                    /* most new edges this blanket can emit */
    int32_t n_new_vert_max;               /* most endpoints over all its new edges */
    int32_t pad_;                         /* scratch doubles the blanket's n-ary (GLC) edges need during assembly */
    int64_t new_off;                      /* arena offset where new-edge records are packed */
    int64_t new_len;                      /* doubles reserved at new_off */
    int64_t out_off;                      /* arena offset of the per-blanket output record */
    int64_t tinfo_off;                    /* arena offset for the target information, or -1 */
} spg_blanket_desc;
typedef struct {
    int64_t off;    /* arena offset of the edge record */
    int32_t len;    /* record length in doubles */
    int32_t kind;   /* SPG_EDGE_* */
    int32_t vbegin; /* into edge_vert[] (local blanket indices) */
    int32_t nv;
} spg_edge_ref;
/* per-blanket output record layout (doubles) at out_off:
 *   [0] status  [1] info bits  [2] kld  [3] min_gap  [4] n_new  [5] ready tag
 *   then per new edge e < n_new: [6+4e] kind  [7+4e] record offset relative to new_off
 *                                [8+4e] record length  [9+4e] nv
 *   then, starting at 6 + 4*n_new_max: the local vertex indices of the new edges, concatenated
 * record length = SPG_OUT_LEN(n_new_max, n_new_vert_max).
 * [5] is written LAST (after a system-scope release) with SPG_READY_WORD(spg_round_desc.tag) — 2^52 + tag,
 * a value no other word of a record can hold, so stale mailbox contents never look ready — once everything the graph
 * update needs (status, n_new, the new-edge table and the new records in the arena) is in place; the
 * per-blanket KLD [2] — and a status change to SPG_ST_KLD_NOT_PD — may land later, at the latest when
 * the launch has completed. A host that polls the mailbox can therefore commit a batch while its
 * KLD tails are still running.
 * When the record is complete (KLD included) the device overwrites [5] with SPG_FINAL_WORD(tag): a poller treats
 * either value as "ready", and FINAL as "this record will not change any more". */
#define SPG_OUT_HDR 6
#define SPG_READY_WORD(tag) (4503599627370496.0 + (double)(tag))
#define SPG_FINAL_WORD(tag) (4503599627370496.0 + 4294967296.0 + (double)(tag))
#define SPG_OUT_LEN(n_new_max, n_new_vert_max) (SPG_OUT_HDR + 4 * (n_new_max) + (n_new_vert_max))
typedef struct {
    const spg_options *opts;
    int32_t n_blankets, first, count;    /* compute blankets [first, first+count) */
    const spg_blanket_desc *blankets;    /* n_blankets */
    const int64_t *vert_pose_off;        /* arena offsets of the blanket vertices' poses */
    const spg_edge_ref *edges;
    const int32_t *edge_vert;
    int64_t n_vert_total, n_edge_total, n_edge_vert_total;
    /* optional host "mailbox": when mail_len > 0 and the backend has one, the out records of the
     * computed blankets are ALSO delivered to backend->mailbox()[out_off - mail_base] (pinned host
     * memory written by the kernel), so the host needs no device->host copy to read them */
    int64_t mail_base, mail_len;
    int32_t slot;   /* launch slot: batches in different slots may be in flight at the same time */
    int32_t tag;    /* launch tag: SPG_READY_WORD(tag) lands in word [5] of every out record of this launch */
} spg_round_desc;
typedef struct {
    void *user;
    void *(*alloc)(void *user, int64_t doubles);
    void (*release)(void *user, void *p);
    int (*upload)(void *user, void *dst, const double *src, int64_t doubles);   /* host -> arena */
    int (*download)(void *user, double *dst, const void *src, int64_t doubles); /* arena -> host */
    int (*run_round)(void *user, void *arena, const spg_round_desc *round);     /* may be asynchronous */
    int (*synchronize)(void *user);
    const double *(*mailbox)(void *user);   /* may be NULL: no mailbox, out records are downloaded */
    /* optional: two launch slots for overlapping the host work of one batch with the device work of
     * another. NULL = the backend runs one batch at a time */
    int (*synchronize_slot)(void *user, int slot);
    const double *(*mailbox_slot)(void *user, int slot);
} spg_backend;
int spg_ctx_create_injected(spg_ctx **out, const spg_backend *backend);

/* oracle-side twin of run_round on host memory (exported by oracle/libspg_ref.so only) */
int spg_run_round(double *arena, const spg_round_desc *round);

#ifdef __cplusplus
}
#endif
#endif /* SPG_H_ */
